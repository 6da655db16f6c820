"""The VAE kernels (``orv_amd/csrc/vae.hip``, the convolution kernels of ``gemm.hip``) one by one against the float64 restatements of
``tests/vae_ref.py``, at the channel widths of the real model (128 / 256 / 256 / 512: 4, 8 and 16 channels per group) and at the
geometries its decoder and encoder dispatch: stride-2 down-sampling with the implied far pad, nearest x2 upsampling in space and
time (all frames doubled / first frame apart), conv_cache frames in front, every N tile of the general implicit-GEMM kernel.

Rules of every test here: a buffer the kernel overwrites is NaN-filled first, memory the kernel must not touch carries a sentinel
compared bit for bit.

Bounds (none of them comes from what the kernels return):
  * im2col is a pure index kernel: bit-exact, zero tail included.
  * convolutions: |err| <= 2^-8 |ref| + K 2^-23 (|A| conv |W| + |bias| + |R|) elementwise: one bf16 rounding of the output + fp32
    accumulation of K exact bf16 products.  For ``randn / sqrt(K)`` weights and K <= 3456 the second term is below 1 % of the output's
    standard deviation; one wrong 64-channel tap line moves an output by sqrt(64 / K) of it.
  * GroupNorm sums: |err| <= L 2^-23 sum|term| with L = 64 + 64 + ceil(nblk / 256) + 8, the longest fp32 addition chain (per thread,
    per group in LDS, per reduce thread, the tree).
  * statistics condition: mean and rstd, derived from the kernel's sums as ``vae_norm_apply_kernel`` derives them, within 2^-10
    (mean: of the std; rstd: relative) of the two-pass float64 values.
  * norm_apply: |err| <= 2^-8 |ref| + 4 A + 1.1 * 2^-10 |n gamma zy|, A = what the float32 CPU evaluation of the same formulas loses
    against float64, the last term what the statistics condition allows.
The measured maxima, as fractions of these bounds, are in ``profiles/vae_kernel_parity.txt`` (``ORV_PARITY_REPORT=<file>`` makes a
run of this module write them).
"""
import functools
import os
import subprocess
import sys

import pytest
import torch

import vae_ref as ref

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
                f.write(f"{k:<52s} {_MEASURED[k]:.4f}\n")


def rb(g, *shape, mul=1.0, add=0.0):
    """bf16-representable random values, as bf16."""
    return (torch.randn(*shape, generator=g) * mul + add).to(BF)


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32).cpu()


def guarded(g, n_elems, guard=256):
    """Flat bf16 buffer of ``n_elems`` NaNs followed by ``guard`` sentinel values -> (buffer, sentinel)."""
    sentinel = rb(g, guard)
    buf = torch.full((n_elems + guard,), NAN, dtype=BF)
    buf[n_elems:] = sentinel
    return buf.to(_dev()), sentinel


# ---------------------------------------------------------------------------------------------------------------------------
# geometries: name -> kt, stride, pad_lo, ups_s, ups_t, t_shift, source (Ts, Hs, Ws) -> output (T, H, W)
# ---------------------------------------------------------------------------------------------------------------------------
def _down(hw):
    return ((hw[0] + 1 - 3) // 2 + 1, (hw[1] + 1 - 3) // 2 + 1)          # pad (0, 1, 0, 1), kernel 3, stride 2


def geometry(name, hw=(5, 7)):
    Hs, Ws = hw
    if name.startswith("causal"):                                        # causal 3x3x3, t_shift conv_cache frames in front
        ts = int(name[-1])
        return (3, 1, 1, 0, 0, ts), (3 + ts, Hs, Ws), (3, Hs, Ws)
    if name == "frame":                                                  # per-frame 3x3
        return (1, 1, 1, 0, 0, 0), (2, Hs, Ws), (2, Hs, Ws)
    if name == "down":
        return (1, 2, 0, 0, 0, 0), (3, Hs, Ws), (3,) + _down(hw)
    if name == "ups":
        return (1, 1, 1, 1, 0, 0), (2, Hs, Ws), (2, 2 * Hs, 2 * Ws)
    if name == "ups_t1":                                                 # all frames doubled
        return (1, 1, 1, 1, 1, 0), (2, Hs, Ws), (4, 2 * Hs, 2 * Ws)
    if name == "ups_t2":                                                 # first frame apart
        return (1, 1, 1, 1, 2, 0), (3, Hs, Ws), (5, 2 * Hs, 2 * Ws)
    raise KeyError(name)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. im2col: bit-exact
# ---------------------------------------------------------------------------------------------------------------------------
IM2COL_GEOS = [("causal0", (5, 7)), ("causal1", (5, 7)), ("causal2", (5, 7)), ("frame", (5, 7)), ("down", (9, 11)), ("down", (8, 10)),
               ("ups", (5, 7)), ("ups_t1", (5, 7)), ("ups_t2", (5, 7))]


@pytest.mark.parametrize("C", [8, 16, 32])
@pytest.mark.parametrize("name,hw", IM2COL_GEOS)
def test_im2col_is_bit_exact_whole_and_in_slabs(name, hw, C):
    """The RGB stem (8), the latent stem (16) and the toy width (32); Kpad the next multiple of 64 and one further; every geometry
    whole, then as three slabs with m0 > 0 and a ragged row count, each into a larger NaN-filled buffer."""
    from orv_amd import ops
    geo, (Ts, Hs, Ws), (T, H, W) = geometry(name, hw)
    kt = geo[0]
    B = 2
    g = torch.Generator().manual_seed(C + T * 7 + H)
    src = rb(g, B, Ts, Hs, Ws, C)
    srcd = src.to(_dev())
    M, K = B * T * H * W, kt * 9 * C
    bad = 0
    for Kpad in ((K + 63) // 64 * 64, (K + 63) // 64 * 64 + 64):
        want = ref.im2col_ref(src, *geo, (T, H, W), Kpad)
        assert bool((want[:, K:] == 0).all())
        cuts = [0, M] if M < 8 else [1, M // 3 + 1, 2 * M // 3 + 3, M]
        for m0, m1 in [(0, M)] + list(zip(cuts[:-1], cuts[1:])):
            mc, lead = m1 - m0, 3
            assert (m0, mc) == (0, M) or (m0 > 0 and mc % 256 != 0)
            buf, sentinel = guarded(g, (lead + mc) * Kpad)
            dst = buf[lead * Kpad:(lead + mc) * Kpad].view(mc, Kpad)
            ops.vae_im2col(srcd, dst, B, Ts, Hs, Ws, C, T, H, W, kt, 3, 3, *geo[1:], Kpad, m0, mc)
            got = buf.cpu()
            assert torch.isnan(got[:lead * Kpad]).all(), "rows in front of the slab were written"
            assert torch.equal(bits(got[(lead + mc) * Kpad:]), bits(sentinel)), "rows behind the slab were written"
            rows = got[lead * Kpad:(lead + mc) * Kpad].view(mc, Kpad)
            assert not torch.isnan(rows).any(), "a chunk of the slab (or of its zero tail) was not written"
            bad += int((bits(rows) != bits(want[m0:m1])).sum())
            assert torch.equal(bits(rows), bits(want[m0:m1])), (name, C, Kpad, m0, mc)
    _note("im2col (mismatching elements)", bad)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. / 3. convolutions: the implicit-GEMM kernels and im2col + GEMM against the same reference
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def conv_case(geo, src_thw, out_thw, B, C, N):
    """Operands (bf16, CPU) and the float64 reference with and without the residual, computed once per shape."""
    kt = geo[0]
    Ts, Hs, Ws = src_thw
    K = kt * 9 * C
    g = torch.Generator().manual_seed(K + N + Ts * 31 + Hs)
    M = B * out_thw[0] * out_thw[1] * out_thw[2]
    c = {"src": rb(g, B, Ts, Hs, Ws, C), "Wp": rb(g, N, K, mul=K ** -0.5), "bias": rb(g, N), "res": rb(g, M, N), "M": M, "K": K}
    c["ref0"] = ref.conv_ref(c["src"], c["Wp"], c["bias"], None, *geo, out_thw)
    c["ref2"] = (c["ref0"][0] + c["res"].double(), c["ref0"][1] + c["res"].double().abs())
    return c


def conv_ok(family, got, want, scale, K):
    got = got.double().cpu()
    assert not torch.isnan(got).any(), (family, "an output element was not written")
    bound = 2.0 ** -8 * want.abs() + K * 2.0 ** -23 * scale
    ratio = ((got - want).abs() / bound.clamp_min(1e-300)).max().item()
    _note(family, ratio)
    assert ratio <= 1.0, (family, ratio)


def run_conv(c, geo, src_thw, out_thw, B, C, N, epi, path):
    """``path`` 'implicit': orv_conv_gemm_bf16; 'patch': orv_vae_im2col + orv_gemm_bf16.  -> out [M, N] (CPU); the rows behind the
    output are checked to be untouched."""
    from orv_amd import ops
    dev = _dev()
    M, K = c["M"], c["K"]
    g = torch.Generator().manual_seed(M + N)
    buf, sentinel = guarded(g, M * N, guard=8 * N)
    out = buf[:M * N].view(M, N)
    R = c["res"].to(dev) if epi == 2 else None
    if path == "implicit":
        ops.conv_gemm(c["src"].to(dev), c["Wp"].to(dev), c["bias"].to(dev), out, B, *src_thw, C, *out_thw, geo[0], 3, 3, *geo[1:], N,
                      R=R, ldr=N)
    else:
        patch = torch.full((M, K), NAN, dtype=BF, device=dev)
        ops.vae_im2col(c["src"].to(dev), patch, B, *src_thw, C, *out_thw, geo[0], 3, 3, *geo[1:], K, 0, M)
        ops.gemm(patch, c["Wp"].to(dev), c["bias"].to(dev), out, M, N, K, epilogue=epi, R=R, ldr=N)
    got = buf.cpu()
    assert torch.equal(bits(got[M * N:]), bits(sentinel)), "rows behind the output were written"
    return got[:M * N].view(M, N)


def check_conv(family, geo, src_thw, out_thw, B, C, N, paths=("implicit", "patch")):
    c = conv_case(geo, src_thw, out_thw, B, C, N)
    for epi in (0, 2):
        want, scale = c[f"ref{epi}"]
        for path in paths:
            got = run_conv(c, geo, src_thw, out_thw, B, C, N, epi, path)
            conv_ok(family if path == "implicit" else "conv im2col + gemm", got, want, scale, c["K"])


GENERAL_GEOS = {"down": (17, 18), "ups": (5, 7), "ups_t1": (5, 7), "ups_t2": (5, 7)}     # M = 432, 560, 1120, 1400


@pytest.mark.parametrize("N", [64, 128, 256])
@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("name", list(GENERAL_GEOS))
def test_general_conv_kernel_non_simple_geometries(name, C, N):
    """conv_gemm_kernel<256, BN, EPI, false>: stride 2 with pad_lo = 0 (H = 17: no far pad line is read; W = 18: one is) and the three
    upsampling forms, one and two 64-channel blocks per tap, every BN, both epilogues, B = 2, ragged last tile.  The same shapes
    through im2col + GEMM meet the same bound."""
    geo, src_thw, out_thw = geometry(name, GENERAL_GEOS[name])
    check_conv("conv general [non-SIMPLE]", geo, src_thw, out_thw, 2, C, N)


SIMPLE_CASES = [  # kt, t_shift, (T, H, W), N
    (3, 0, (3, 40, 2), 64), (3, 2, (3, 40, 2), 64),            # conv_out: BN = 64, W = 2 (every voxel an x edge), M = 480
    (3, 1, (3, 70, 1), 128), (1, 0, (3, 70, 1), 128),          # W = 1 fails the strip kernel's W >= 2, M = 420
    (3, 0, (2, 150, 1), 256),
]


@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("kt,t_shift,thw,N", SIMPLE_CASES)
def test_general_conv_kernel_simple_form_in_process(kt, t_shift, thw, N, C):
    """conv_gemm_kernel<256, BN, EPI, true> where the dispatch takes it without a switch: N = 64, and W = 1."""
    T, H, W = thw
    check_conv("conv general [SIMPLE]", (kt, 1, 1, 0, 0, t_shift), (T + t_shift, H, W), thw, 2, C, N)


CHILD_CASES = [  # kt, t_shift, B, (T, H, W): ordinary stride-1 shapes, the strip kernel's when ORV_CONV_STRIP is unset
    (3, 0, 2, (3, 9, 11)),          # M = 594: three tiles, the last ragged, tiles cross rows, frames and batch elements
    (3, 2, 1, (4, 9, 8)),           # conv_cache frames in front, M = 288
    (1, 0, 2, (2, 20, 17)),         # per-frame, M = 680
]


def _child_main():
    """ORV_CONV_STRIP=0 is read once per process: the SIMPLE form at N = 128 / 256 on ordinary shapes, in this (fresh) process.
    The first mismatch or HIP error ends the process with a non-zero status."""
    n = 0
    for kt, t_shift, B, thw in CHILD_CASES:
        for C in (64, 128):
            for N in (128, 256):
                T, H, W = thw
                check_conv("conv general [SIMPLE, ORV_CONV_STRIP=0]", (kt, 1, 1, 0, 0, t_shift), (T + t_shift, H, W), thw, B, C, N,
                           paths=("implicit",))
                n += 1
    torch.cuda.synchronize()
    for k, v in _MEASURED.items():
        print(f"CHILD-PARITY {v:.6f} {k}")
    print(f"CHILD-OK {n}")


def test_general_conv_kernel_simple_form_at_the_strip_shapes_in_a_child_process():
    """One fresh child with ORV_CONV_STRIP=0 and its own time limit; an abnormal exit status fails the test and nothing further is started."""
    env = dict(os.environ, ORV_CONV_STRIP="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and f"CHILD-OK {len(CHILD_CASES) * 4}" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    for line in r.stdout.splitlines():
        if line.startswith("CHILD-PARITY "):
            _, v, k = line.split(" ", 2)
            _note(k, float(v))


STRIP_CASES = [  # B, T, H, W, Cin, Cout, kt, t_shift: the small-M shapes of test_gpu_vae.test_conv_kernels_against_torch_conv3d
    (2, 3, 5, 7, 64, 128, 3, 0), (1, 4, 9, 2, 128, 128, 3, 2), (1, 2, 20, 33, 64, 256, 1, 0), (3, 1, 16, 16, 192, 128, 3, 0),
]


@pytest.mark.parametrize("B,T,H,W,C,N,kt,t_shift", STRIP_CASES)
def test_strip_conv_kernel_128x128_tile(B, T, H, W, C, N, kt, t_shift):
    """conv_strip_kernel<128, 128>: every grid below half of the CUs.  (C = 192, kt = 3 has K = 5184: the accumulation term of the
    bound grows with K, it is 1.5 % of the output's standard deviation there.)"""
    check_conv("conv strip 128x128", (kt, 1, 1, 0, 0, t_shift), (T + t_shift, H, W), (T, H, W), B, C, N, paths=("implicit",))


def test_strip_conv_kernel_256x128_tile():
    """conv_strip_kernel<256, 128>: N = 512 and 33 row tiles (132 column tiles of 128 >= half of the CUs, 66 of 256 are not);
    M = 8200 leaves 8 rows to the last tile."""
    B, T, H, W, C, N = 2, 2, 41, 50, 64, 512
    assert torch.cuda.get_device_properties(0).multi_processor_count == 256
    check_conv("conv strip 256x128", (1, 1, 1, 0, 0, 0), (T, H, W), (T, H, W), B, C, N, paths=("implicit",))


# ---------------------------------------------------------------------------------------------------------------------------
# 4. GroupNorm statistics
# ---------------------------------------------------------------------------------------------------------------------------
G = 32
WIDTHS = [32, 64, 128, 256, 512]


def vox_per_block(C):
    return (256 // (C // 8)) * 64


def gn_data(g, B, N, C):
    """Every group has its own mean (g - 16): a wrong channel-to-group assignment is an O(1) error of the sum."""
    mean = (torch.arange(C) // (C // G) - 16).float()
    return (torch.randn(B, N, C, generator=g) + mean).to(BF)


def sums_ok(got, x, nblk):
    r = ref.groupnorm_sums_ref(x, G)
    L = 64 + 64 + -(-nblk // 256) + 8
    got = got.double().cpu()
    assert torch.isfinite(got).all()
    for fam, col, want, scale in (("gn sums [sum]", 0, r["sum"], r["abs"]), ("gn sums [sum of squares]", 1, r["sumsq"], r["sumsq"])):
        ratio = ((got[..., col] - want).abs() / (L * 2.0 ** -23 * scale).clamp_min(1e-300)).max().item()
        _note(fam, ratio)
        assert ratio <= 1.0, (fam, ratio)


def run_sums(x):
    from orv_amd import ops
    B, N, C = x.shape
    return ops.vae_groupnorm_stats(x, B, N, C, G).cpu()


@pytest.mark.parametrize("C", WIDTHS)
def test_groupnorm_sums_at_every_width_and_block_edge(C):
    """1, 2, 4, 8 and 16 channels per group (vstep 64 ... 4); N around the voxels-per-block edge and several blocks with a ragged
    last one; deterministic; batch element 1 alone gives batch element 1's bits."""
    vpb = vox_per_block(C)
    g = torch.Generator().manual_seed(C)
    for N in (1, vpb - 1, vpb, vpb + 1, 3 * vpb + 5):
        x = gn_data(g, 2, N, C)
        xd = x.to(_dev())
        got = run_sums(xd)
        sums_ok(got, x, -(-N // vpb))
        assert torch.equal(bits(got), bits(run_sums(xd))), "two runs differ"
        assert torch.equal(bits(got[1:]), bits(run_sums(xd[1:].contiguous()))), "batch element 1 depends on batch element 0"


@pytest.mark.parametrize("C", [32, 512])
def test_groupnorm_sums_reduce_kernel_second_stride(C):
    """257 block partials + 3 voxels: vae_gn_reduce_kernel's strided loop runs twice for thread 0 and 1 (about 67 MB, B = 1)."""
    N = 257 * vox_per_block(C) + 3
    x = gn_data(torch.Generator().manual_seed(C + 1), 1, N, C)
    xd = x.to(_dev())
    got = run_sums(xd)
    sums_ok(got, x, 258)
    assert torch.equal(bits(got), bits(run_sums(xd))), "two runs differ"


# ---------------------------------------------------------------------------------------------------------------------------
# 5. statistics + norm_apply against the two-pass float64 reference
# ---------------------------------------------------------------------------------------------------------------------------
T_PAIRS = [(1, 1), (2, 2), (4, 2), (8, 2), (3, 3), (5, 3), (9, 3), (9, 9)]
RATIOS = [1, 2, 4, 8]
EPS = 1e-6


def norm_data(g, B, T, H, W, C, ratio):
    """``ratio`` 0: zero-mean; else group g has mean / std = ratio * g / 31 (before the bf16 rounding) and a std in [0.5, 2]."""
    cpg = C // G
    grp = torch.arange(C) // cpg
    std = 0.5 + 1.5 * torch.rand(G, generator=g)[grp]
    x = torch.randn(B, T, H, W, C, generator=g)
    if ratio:
        x = x + (ratio * grp / 31.0)
    return (x * std).to(BF)


def kernel_statistics(sums, n):
    """mean and rstd as vae_norm_apply_kernel derives them from the sums, in float32."""
    inv_n = torch.ones((), dtype=F32) / torch.tensor(float(n), dtype=F32)
    mean = sums[..., 0] * inv_n
    var = (sums[..., 1] * inv_n - mean * mean).clamp_min(0.0)
    return mean, torch.rsqrt(var + torch.tensor(EPS, dtype=F32))


@pytest.mark.parametrize("T,Tz", T_PAIRS)
@pytest.mark.parametrize("C", WIDTHS)
def test_stats_and_norm_apply_against_two_pass_float64(C, T, Tz):
    """Every width x every (T, Tz) pair; the spatial ratio H / hz (latent 3 x 5; 3 x 10 at ratio 1 so that W >= 10 and C = 512 spans
    several blocks in x) and the options rotate with the case so that every width meets every ratio and every option pair:
    zero-mean and ratio-16 data, decoder (zy / zb) and encoder form, SiLU on / off, out_lead 0 / 2 with the lead frames a sentinel."""
    from orv_amd import ops
    dev = _dev()
    ic, it = WIDTHS.index(C), T_PAIRS.index((T, Tz))
    r = RATIOS[(ic + it) % 4]
    a, b = (it // 4 + ic // 2) % 2, (it // 2 + ic) % 2                    # (ratio, a, b) takes all 16 values over the 40 cases
    hz, wz = (3, 10) if r == 1 else (3, 5)
    B, H, W = 2, hz * r, wz * r
    assert W >= 10
    g = torch.Generator().manual_seed(C * 100 + T * 10 + Tz)
    gamma, beta = rb(g, C, mul=0.2, add=1.0), rb(g, C, mul=0.1)
    zy, zb = rb(g, B, Tz, hz, wz, C, mul=0.3, add=1.0), rb(g, B, Tz, hz, wz, C, mul=0.3)
    n = T * H * W * (C // G)
    runs = [  # data ratio, decoder form, silu, out_lead
        (0, True, a, 2 * b), (16, True, 1 - a, 2 - 2 * b), (16 if a else 0, False, b, 2 * a),
    ]
    data = {ratio: norm_data(g, B, T, H, W, C, ratio) for ratio in (0, 16)}
    sums = {}
    for ratio, x in data.items():
        sums[ratio] = ops.vae_groupnorm_stats(x.to(dev), B, T * H * W, C, G)
        # (a) the statistics condition
        want = ref.norm_apply_ref(x, gamma, beta, G, EPS)
        mean, rstd = kernel_statistics(sums[ratio].cpu(), n)
        e_mean = ((mean.double() - want["mean"]).abs() / want["std"]).max().item() / 2.0 ** -10
        e_rstd = ((rstd.double() - want["rstd"]).abs() / want["rstd"]).max().item() / 2.0 ** -10
        _note(f"gn stats condition [mean, ratio {ratio}]", e_mean)
        _note(f"gn stats condition [rstd, ratio {ratio}]", e_rstd)
        assert e_mean <= 1.0 and e_rstd <= 1.0, (ratio, e_mean, e_rstd)
    for ratio, decoder, silu, lead in runs:
        x = data[ratio]
        z = (zy, zb) if decoder else (None, None)
        r64 = ref.norm_apply_ref(x, gamma, beta, G, EPS, *z, silu=bool(silu))
        r32 = ref.norm_apply_ref(x.float(), gamma.float(), beta.float(), G, EPS, *(None if t is None else t.float() for t in z),
                                 silu=bool(silu), dtype=F32)
        per = (lead + T) * H * W * C
        buf, tail = guarded(g, B * per)
        out = buf[:B * per].view(B, lead + T, H, W, C)
        head = rb(g, B, lead, H, W, C)
        out[:, :lead] = head.to(dev)
        zd = [None if t is None else t.to(dev) for t in z]
        ops.vae_norm_apply(x.to(dev), out, sums[ratio], gamma.to(dev), beta.to(dev), zd[0], zd[1], B, T, H, W, C, G,
                           Tz if decoder else 0, hz if decoder else 0, wz if decoder else 0, EPS, silu, lead)
        got_all = buf.cpu()
        assert torch.equal(bits(got_all[B * per:]), bits(tail)), "memory behind the output was written"
        got_all = got_all[:B * per].view(B, lead + T, H, W, C)
        assert torch.equal(bits(got_all[:, :lead]), bits(head)), "the lead frames were written"
        got = got_all[:, lead:].double()
        assert not torch.isnan(got).any(), "an output element was not written"
        A = (r32["out"].double() - r64["out"]).abs().max().item()
        bound = 2.0 ** -8 * r64["out"].abs() + 4 * A + 1.1 * 2.0 ** -10 * r64["gain"].abs()
        ratio_b = ((got - r64["out"]).abs() / bound).max().item()
        _note(f"norm_apply [ratio {ratio}]", ratio_b)
        assert ratio_b <= 1.0, (ratio, decoder, silu, lead, ratio_b, A)


if __name__ == "__main__":
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    _child_main()
