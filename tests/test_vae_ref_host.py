"""Host checks of ``tests/vae_ref.py``: the float64 restatements the GPU tests measure the VAE kernels against are themselves
compared with the CPU oracle's modules (``oracle/vae.py``), ``torch.nn.GroupNorm`` and ``F.interpolate``, all in float64, so a
mistake in a restatement cannot pass as a kernel check.  No GPU, no ``orv_amd`` import."""
import pytest
import torch
import torch.nn.functional as F

import vae_ref as ref
from oracle import vae as ovae

F64 = torch.float64
TIGHT = dict(rtol=1e-11, atol=1e-11)


def _cl(x):
    """[B, C, T, H, W] -> channels-last [B, T, H, W, C]"""
    return x.permute(0, 2, 3, 4, 1).contiguous()


def _pack(w):
    """conv weight [N, C, (kt,) 3, 3] -> [N, taps * C], column = ((dt * 3 + dy) * 3 + dx) * C + ci"""
    if w.ndim == 4:
        w = w[:, :, None]
    return w.permute(0, 2, 3, 4, 1).reshape(w.shape[0], -1).contiguous()


def _flat(y):
    return _cl(y).reshape(-1, y.shape[1])


@pytest.mark.parametrize("kt", [1, 3])
def test_conv_ref_is_the_causal_conv_with_first_frame_padding_and_with_a_conv_cache(kt):
    torch.manual_seed(kt)
    m = ovae.CogVideoXCausalConv3d(8, 5, (kt, 3, 3)).double()
    x = torch.randn(2, 8, 4, 5, 7, dtype=F64)
    res = torch.randn(2 * 4 * 5 * 7, 5, dtype=F64)
    want = _flat(m(x)) + res
    got, scale = ref.conv_ref(_cl(x), _pack(m.conv.weight.detach()), m.conv.bias.detach(), res, kt, 1, 1, 0, 0, 0, (4, 5, 7))
    assert torch.allclose(got, want, **TIGHT) and bool((scale >= got.abs() - 1e-12).all())
    if kt == 3:          # second frame batch: the previous batch's last kt - 1 frames stand in front (t_shift); one frame: copy + cache
        for t_shift in (1, 2):
            prev = torch.randn(2, 8, 2, 5, 7, dtype=F64)
            # t_shift = 1: the kernel sees [prev[-1], x] and replicates ITS first frame once more: a cache of two copies of prev[-1]
            cache = prev if t_shift == 2 else prev[:, :, 1:].expand(-1, -1, 2, -1, -1)
            want = _flat(m(x, ovae.ConvCache({id(m): cache})))
            src = torch.cat([prev[:, :, 2 - t_shift:], x], dim=2)
            got, _ = ref.conv_ref(_cl(src), _pack(m.conv.weight.detach()), m.conv.bias.detach(), None, 3, 1, 1, 0, 0, t_shift, (4, 5, 7))
            assert torch.allclose(got, want, **TIGHT), t_shift


@pytest.mark.parametrize("T,compress", [(2, True), (4, True), (3, True), (5, True), (1, True), (3, False)])
def test_conv_ref_is_the_upsample_block(T, compress):
    torch.manual_seed(T)
    m = ovae.CogVideoXUpsample3D(8, 6, compress_time=compress).double()
    x = torch.randn(2, 8, T, 3, 5, dtype=F64)
    want = m(x)
    ups_t, To = 0, T
    if compress and T > 1:
        ups_t, To = (2, 1 + 2 * (T - 1)) if T % 2 else (1, 2 * T)
    assert want.shape[2:] == (To, 6, 10)
    got, _ = ref.conv_ref(_cl(x), _pack(m.conv.weight.detach()), m.conv.bias.detach(), None, 1, 1, 1, 1, ups_t, 0, (To, 6, 10))
    assert torch.allclose(got, _flat(want), **TIGHT)


@pytest.mark.parametrize("Hs,Ws", [(9, 11), (8, 10), (9, 10)])
def test_conv_ref_is_the_spatial_part_of_the_downsample_block(Hs, Ws):
    torch.manual_seed(Hs)
    m = ovae.CogVideoXDownsample3D(8, 6, compress_time=False).double()          # the time average stays host glue in vae.py
    x = torch.randn(2, 8, 3, Hs, Ws, dtype=F64)
    want = m(x)
    Ho, Wo = (Hs + 1 - 3) // 2 + 1, (Ws + 1 - 3) // 2 + 1
    assert want.shape[2:] == (3, Ho, Wo)
    got, _ = ref.conv_ref(_cl(x), _pack(m.conv.weight.detach()), m.conv.bias.detach(), None, 1, 2, 0, 0, 0, 0, (3, Ho, Wo))
    assert torch.allclose(got, _flat(want), **TIGHT)


GEOMETRIES = [  # kt, stride, pad_lo, ups_s, ups_t, t_shift, (Ts, Hs, Ws), (T, H, W)
    (3, 1, 1, 0, 0, 0, (3, 5, 7), (3, 5, 7)), (3, 1, 1, 0, 0, 1, (4, 5, 7), (3, 5, 7)), (3, 1, 1, 0, 0, 2, (5, 5, 7), (3, 5, 7)),
    (1, 1, 1, 0, 0, 0, (2, 5, 7), (2, 5, 7)), (1, 2, 0, 0, 0, 0, (2, 9, 11), (2, 4, 5)), (1, 2, 0, 0, 0, 0, (2, 8, 10), (2, 4, 5)),
    (1, 1, 1, 1, 0, 0, (2, 5, 7), (2, 10, 14)), (1, 1, 1, 1, 1, 0, (2, 5, 7), (4, 10, 14)), (1, 1, 1, 1, 2, 0, (3, 5, 7), (5, 10, 14)),
]


@pytest.mark.parametrize("geo", GEOMETRIES)
def test_im2col_ref_times_the_packed_weight_is_conv_ref(geo):
    kt, stride, pad_lo, ups_s, ups_t, t_shift, (Ts, Hs, Ws), thw = geo
    g = torch.Generator().manual_seed(sum(thw) + t_shift)
    C, N = 8, 4
    src = torch.randn(2, Ts, Hs, Ws, C, generator=g, dtype=F64)
    K = kt * 9 * C
    Kpad = (K + 63) // 64 * 64 + 64
    Wp = torch.zeros(N, Kpad, dtype=F64)
    Wp[:, :K] = torch.randn(N, K, generator=g, dtype=F64)
    want, _ = ref.conv_ref(src, Wp[:, :K], None, None, kt, stride, pad_lo, ups_s, ups_t, t_shift, thw)
    patch = ref.im2col_ref(src, kt, stride, pad_lo, ups_s, ups_t, t_shift, thw, Kpad)
    assert patch.shape == (want.shape[0], Kpad) and bool((patch[:, K:] == 0).all())
    assert torch.allclose(patch @ Wp.T, want, **TIGHT)
    M = want.shape[0]
    m0, mc = M // 3 + 1, M // 2
    assert torch.equal(ref.im2col_ref(src, kt, stride, pad_lo, ups_s, ups_t, t_shift, thw, Kpad, m0, mc), patch[m0:m0 + mc])


T_PAIRS = [(1, 1), (2, 2), (4, 2), (8, 2), (3, 3), (5, 3), (9, 3), (9, 9)]


def test_integer_nearest_index_formulas_are_f_interpolate():
    for n_in in (3, 5, 10):
        for r in (1, 2, 4, 8):
            src = torch.arange(n_in, dtype=F64)[None, None]
            want = F.interpolate(src, size=n_in * r)[0, 0].long().tolist()
            assert ref.nearest_index(n_in * r, n_in) == want
    for T, Tz in T_PAIRS:
        z = torch.arange(Tz, dtype=F64)[None, None, :, None, None]
        if T > 1 and T % 2 == 1:          # CogVideoXSpatialNorm3D: first frame apart
            want = torch.cat([F.interpolate(z[:, :, :1], size=(1, 1, 1)), F.interpolate(z[:, :, 1:], size=(T - 1, 1, 1))], dim=2)
        else:
            want = F.interpolate(z, size=(T, 1, 1))
        assert ref.latent_time_index(T, Tz) == want.flatten().long().tolist(), (T, Tz)
    # the frame lists of the time upsampling (CogVideoXUpsample3D)
    for Ts in (2, 3, 4, 5):
        x = torch.arange(Ts, dtype=F64)[None, None, :, None, None]
        if Ts % 2 == 1:
            want = torch.cat([x[:, :, :1], F.interpolate(x[:, :, 1:], scale_factor=(2.0, 1.0, 1.0))], dim=2)
        else:
            want = F.interpolate(x, scale_factor=(2.0, 1.0, 1.0))
        assert ref.upsampled_frames(Ts, 2 if Ts % 2 else 1) == want.flatten().long().tolist()


@pytest.mark.parametrize("T,Tz", T_PAIRS)
@pytest.mark.parametrize("r", [1, 2, 4, 8])
def test_norm_apply_ref_is_the_spatial_norm(T, Tz, r):
    torch.manual_seed(T * 10 + r)
    C, G, hz, wz = 64, 32, 3, 5
    m = ovae.CogVideoXSpatialNorm3D(C, 16, G).double()
    m.norm_layer.weight.data.normal_(1, 0.2), m.norm_layer.bias.data.normal_(0, 0.2)
    f = torch.randn(2, C, T, hz * r, wz * r, dtype=F64) * 3 + 2
    zq = torch.randn(2, 16, Tz, hz, wz, dtype=F64)
    want = _cl(m(f, zq))
    zy, zb = _cl(m.conv_y(zq)), _cl(m.conv_b(zq))          # 1x1x1 convolutions commute with the nearest resize
    got = ref.norm_apply_ref(_cl(f), m.norm_layer.weight.detach(), m.norm_layer.bias.detach(), G, 1e-6, zy.detach(), zb.detach())
    assert torch.allclose(got["out"], want, rtol=1e-10, atol=1e-10)
    silu = ref.norm_apply_ref(_cl(f), m.norm_layer.weight.detach(), m.norm_layer.bias.detach(), G, 1e-6, zy.detach(), zb.detach(), silu=True)
    assert torch.allclose(silu["out"], F.silu(want), rtol=1e-10, atol=1e-10)


@pytest.mark.parametrize("C", [32, 128, 512])
def test_norm_apply_ref_is_group_norm(C):
    torch.manual_seed(C)
    gn = torch.nn.GroupNorm(32, C, eps=1e-6).double()
    gn.weight.data.normal_(1, 0.2), gn.bias.data.normal_(0, 0.2)
    f = torch.randn(2, C, 3, 4, 5, dtype=F64) * 2 + torch.arange(C, dtype=F64)[None, :, None, None, None] / 8
    got = ref.norm_apply_ref(_cl(f), gn.weight.detach(), gn.bias.detach(), 32, 1e-6)
    assert torch.allclose(got["out"], _cl(gn(f)), rtol=1e-10, atol=1e-10)
    # the pieces the GPU bound is built from
    xg = _cl(f).reshape(2, -1, 32, C // 32)
    assert torch.allclose(got["mean"], xg.mean((1, 3))) and torch.allclose(got["std"], xg.var((1, 3), unbiased=False).sqrt())
    assert torch.allclose(got["n"] * gn.weight.detach(), got["gain"])
    sums = ref.groupnorm_sums_ref(_cl(f).reshape(2, -1, C), 32)
    n = xg.shape[1] * xg.shape[3]
    assert torch.allclose(sums["sum"] / n, got["mean"]) and torch.allclose(sums["sumsq"] / n - got["mean"] ** 2, got["std"] ** 2)
    assert bool((sums["abs"] >= sums["sum"].abs()).all())
    # the float32 evaluation is the same function, a float32 away
    got32 = ref.norm_apply_ref(_cl(f).float(), gn.weight.detach().float(), gn.bias.detach().float(), 32, 1e-6, dtype=torch.float32)
    assert got32["out"].dtype == torch.float32 and torch.allclose(got32["out"].double(), got["out"], rtol=1e-4, atol=1e-4)
