"""Explicit float64 restatements of the VAE kernels (CPU only; nothing here imports the GPU library).

``tests/test_vae_ref_host.py`` anchors every function against the CPU oracle's modules (``oracle/vae.py``), ``torch.nn.GroupNorm``
and ``F.interpolate`` in float64; the GPU tests (``tests/test_gpu_vae_kernels.py``) compare the kernels with them.  Activations are
channels-last ``[B, T, H, W, C]`` and hold the (bf16-representable) values the kernel reads; ``dtype`` selects the precision the
formulas are evaluated in (float64: the reference; float32: the yardstick for what plain fp32 evaluation of the same formulas loses).

A convolution geometry is the tuple of the kernel ABI: ``kt`` temporal taps (3 x 3 in space), spatial ``stride``, ``pad_lo`` zero
lines in front (the far side is implied by the output size), ``ups_s`` (nearest x2 in H, W), ``ups_t`` (0 none, 1 all frames doubled,
2 first frame kept apart + the others doubled), ``t_shift`` context frames the caller put in front of the source.
"""
import torch
import torch.nn.functional as F

KH = KW = 3


# ---------------------------------------------------------------------------------------------------------------------------
# index lists
# ---------------------------------------------------------------------------------------------------------------------------
def nearest_index(n_out, n_in):
    """Source index of every output position of a nearest-neighbour resize: floor(i * n_in / n_out), in integers."""
    return [(i * n_in) // n_out for i in range(n_out)]


def latent_time_index(T, Tz):
    """Latent frame every feature frame looks at (SpatialNorm): an odd clip of more than one frame resizes its first frame apart."""
    if T > 1 and T % 2 == 1:
        return [0] + [1 + ((t - 1) * (Tz - 1)) // (T - 1) for t in range(1, T)]
    return nearest_index(T, Tz)


def upsampled_frames(Ts, ups_t):
    """Source frame of every frame of the time-upsampled clip."""
    if ups_t == 0:
        return list(range(Ts))
    if ups_t == 1:
        return [i // 2 for i in range(2 * Ts)]
    return [0] + [1 + (i - 1) // 2 for i in range(1, 1 + 2 * (Ts - 1))]


# ---------------------------------------------------------------------------------------------------------------------------
# convolution
# ---------------------------------------------------------------------------------------------------------------------------
def conv_input(src, kt, stride, pad_lo, ups_s, ups_t, t_shift, out_thw, dtype=torch.float64):
    """The tensor the convolution slides over, built explicitly: ``src`` [B, Ts, Hs, Ws, C] -> [B, C, T + kt - 1, Hp, Wp] such that a
    plain (unpadded) conv3d with stride (1, s, s) yields exactly ``out_thw``."""
    T, H, W = out_thw
    x = src.to(dtype)
    B, Ts, Hs, Ws, C = x.shape
    if ups_s:
        x = x[:, :, [i // 2 for i in range(2 * Hs)]][:, :, :, [i // 2 for i in range(2 * Ws)]]
    frames = upsampled_frames(Ts, ups_t)
    # conv-input frame j = t + dt stands for frame j + t_shift - (kt - 1) of the (upsampled) clip; in front of it: copies of frame 0
    want = [max(j + t_shift - (kt - 1), 0) for j in range(T + kt - 1)]
    assert want[-1] < len(frames), "the output asks for frames the source does not have"
    x = x[:, [frames[j] for j in want]]
    Hi, Wi = x.shape[2], x.shape[3]
    back_h = (H - 1) * stride + KH - pad_lo - Hi
    back_w = (W - 1) * stride + KW - pad_lo - Wi
    assert back_h >= 0 and back_w >= 0, "the output does not cover the input"
    x = x.permute(0, 4, 1, 2, 3)
    return F.pad(x, (pad_lo, back_w, pad_lo, back_h))


def unpack_weight(Wp, C, kt):
    """[N, taps * C] with column ((dt * 3 + dy) * 3 + dx) * C + ci  ->  conv3d weight [N, C, kt, 3, 3]."""
    N = Wp.shape[0]
    return Wp[:, :kt * KH * KW * C].reshape(N, kt, KH, KW, C).permute(0, 4, 1, 2, 3)


def conv_ref(src, Wp, bias, res, kt, stride, pad_lo, ups_s, ups_t, t_shift, out_thw, dtype=torch.float64):
    """-> (out [M, N], scale [M, N]): the convolution + bias + residual, and |A| conv |W| + |bias| + |R| (what an accumulation
    error is measured against).  ``res`` [M, N] or None."""
    C = src.shape[-1]
    N = Wp.shape[0]
    xin = conv_input(src, kt, stride, pad_lo, ups_s, ups_t, t_shift, out_thw, dtype)
    w = unpack_weight(Wp.to(dtype), C, kt)
    out = F.conv3d(xin, w, stride=(1, stride, stride))
    scale = F.conv3d(xin.abs(), w.abs(), stride=(1, stride, stride))
    assert tuple(out.shape[2:]) == tuple(out_thw), (out.shape, out_thw)
    flat = lambda t: t.permute(0, 2, 3, 4, 1).reshape(-1, N)
    out, scale = flat(out), flat(scale)
    if bias is not None:
        out, scale = out + bias.to(dtype), scale + bias.to(dtype).abs()
    if res is not None:
        out, scale = out + res.to(dtype), scale + res.to(dtype).abs()
    return out, scale


def im2col_ref(src, kt, stride, pad_lo, ups_s, ups_t, t_shift, out_thw, Kpad, m0=0, mc=None):
    """Rows [m0, m0 + mc) of the patch matrix by pure indexing, in the dtype of ``src``: row = voxel (b, t, y, x) of the output grid,
    column = tap * C + ci, columns [taps * C, Kpad) zero."""
    T, H, W = out_thw
    B, Ts, Hs, Ws, C = src.shape
    mc = B * T * H * W - m0 if mc is None else mc
    m = torch.arange(m0, m0 + mc)
    x, y, t, b = m % W, (m // W) % H, (m // (W * H)) % T, m // (W * H * T)
    tap = torch.arange(kt * KH * KW)
    dx, dy, dt = tap % KW, (tap // KW) % KH, tap // (KW * KH)
    ti = (t[:, None] + t_shift - (kt - 1) + dt[None]).clamp_min(0)
    yi = y[:, None] * stride - pad_lo + dy[None]
    xi = x[:, None] * stride - pad_lo + dx[None]
    Hi, Wi = (2 * Hs, 2 * Ws) if ups_s else (Hs, Ws)
    ok = (yi >= 0) & (yi < Hi) & (xi >= 0) & (xi < Wi)
    if ups_s:
        yi, xi = yi // 2, xi // 2
    ts = torch.tensor(upsampled_frames(Ts, ups_t))[ti]
    vox = ((b[:, None] * Ts + ts) * Hs + yi.clamp(0, Hs - 1)) * Ws + xi.clamp(0, Ws - 1)
    rows = src.reshape(-1, C)[vox]                                         # [mc, taps, C]
    rows = torch.where(ok[:, :, None], rows, torch.zeros((), dtype=src.dtype))
    out = torch.zeros(mc, Kpad, dtype=src.dtype)
    out[:, :tap.numel() * C] = rows.reshape(mc, -1)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# GroupNorm / SpatialNorm
# ---------------------------------------------------------------------------------------------------------------------------
def groupnorm_sums_ref(x, G, dtype=torch.float64):
    """x [B, N, C] -> dict of [B, G]: ``sum``, ``sumsq`` and ``abs`` (sum of |x|: the scale of the sum's accumulation error; the
    squares are their own)."""
    B, N, C = x.shape
    xg = x.to(dtype).reshape(B, N, G, C // G)
    return {"sum": xg.sum((1, 3)), "sumsq": (xg * xg).sum((1, 3)), "abs": xg.abs().sum((1, 3))}


def norm_apply_ref(x, gamma, beta, G, eps, zy=None, zb=None, silu=False, dtype=torch.float64):
    """Two-pass GroupNorm over (T, H, W, C / G) of x [B, T, H, W, C], affine, then ``* zy[idx] + zb[idx]`` (zy, zb at latent resolution
    [B, Tz, hz, wz, C], looked up by the nearest-resize index lists), then SiLU.  -> dict: ``out``, the normalised value ``n``, the
    gain ``n * gamma * zy`` that a relative error of the statistics is multiplied by, ``mean`` / ``rstd`` / ``std`` [B, G]."""
    B, T, H, W, C = x.shape
    xg = x.to(dtype).reshape(B, T, H, W, G, C // G)
    mean = xg.mean((1, 2, 3, 5), keepdim=True)
    var = ((xg - mean) ** 2).mean((1, 2, 3, 5), keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    n = ((xg - mean) * rstd).reshape(B, T, H, W, C)
    gain = n * gamma.to(dtype)
    out = gain + beta.to(dtype)
    if zy is not None:
        _, Tz, hz, wz, _ = zy.shape
        it, iy, ix = latent_time_index(T, Tz), nearest_index(H, hz), nearest_index(W, wz)
        look = lambda z: z.to(dtype)[:, it][:, :, iy][:, :, :, ix]
        gain = gain * look(zy)
        out = out * look(zy) + look(zb)
    if silu:
        out = out * torch.sigmoid(out)
    return {"out": out, "n": n, "gain": gain, "mean": mean.reshape(B, G), "rstd": rstd.reshape(B, G),
            "std": torch.sqrt(var).reshape(B, G)}
