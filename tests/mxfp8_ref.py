"""CPU restatement of the MXFP8 format of the opt-in MXFP8 inference mode (include/orv_mi355.h "MXFP8"), written from the rule and not
from the kernels: blocks of 32 consecutive elements along the last axis, e4m3fn elements, one e8m0 scale byte 2^e per block with e the
smallest integer such that amax / 2^e <= 448, clamped to [-127, 127]; amax == 0 -> e = 0 (byte 0x7F); element = x / 2^e rounded to
nearest-even in e4m3fn, saturated to +-448.  The input is always the bf16 value.

``quantize`` gives the bytes (torch's float8_e4m3fn / e8m0 conversions, CPU); ``fake_quant`` gives the dequantised values by plain fp32
arithmetic on any device (the emulated-MXFP8 oracle of the model tests).  The known-answer test holds the two to each other."""
import torch

E4M3 = torch.float8_e4m3fn
E8M0 = torch.float8_e8m0fnu


def block_exp(amax: torch.Tensor) -> torch.Tensor:
    """e of the rule for a tensor of block maxima (fp32, >= 0): amax = m 2^p with m in [0.5, 1), and amax / 448 = (m / 0.875) 2^(p - 9),
    so e = p - 9 when m <= 0.875 and p - 8 otherwise."""
    m, p = torch.frexp(amax.float())
    e = torch.where(m <= 0.875, p - 9, p - 8)
    e = torch.where(amax == 0, torch.zeros_like(e), e)
    return e.clamp(-127, 127).to(torch.int32)


def _blocks(x: torch.Tensor) -> torch.Tensor:
    x = x.to(torch.bfloat16).float()
    assert x.shape[-1] % 32 == 0
    return x.reshape(*x.shape[:-1], x.shape[-1] // 32, 32)


def quantize(x: torch.Tensor):
    """-> (q uint8 [..., K], s uint8 [..., K / 32]) on the CPU."""
    xb = _blocks(x.cpu())
    e = block_exp(xb.abs().amax(-1))
    y = (xb.double() * torch.pow(2.0, -e.double())[..., None]).float().clamp(-448.0, 448.0)
    q = y.to(E4M3).view(torch.uint8).reshape(*xb.shape[:-2], -1)
    s = (e + 127).to(torch.uint8)             # e8m0 byte: value 2^(s - 127)
    return q, s


def dequantize(q: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """float64 values of (q, s) (float64: a block scale up to 2^127 times 448 leaves the fp32 range)."""
    v = q.cpu().view(E4M3).double().reshape(*q.shape[:-1], -1, 32)
    return (v * torch.pow(2.0, s.cpu().double() - 127.0)[..., None]).reshape(q.shape)


def fake_quant(x: torch.Tensor) -> torch.Tensor:
    """Dequantised MXFP8 of bf16(x), fp32, on x's device: the element grid of e4m3 at y = x / 2^e is 2^(max(E, -6) - 3) (E = exponent of
    |y|), rounded half to even (torch.round)."""
    xb = _blocks(x)
    e = block_exp(xb.abs().amax(-1)).float()[..., None]
    y = xb * torch.pow(2.0, -e)
    _, p = torch.frexp(y)                       # |y| = m 2^p, m in [0.5, 1): exponent E = p - 1
    step = torch.pow(2.0, (p - 1).clamp(min=-6).float() - 3.0)
    yq = (torch.round(y / step) * step).clamp(-448.0, 448.0)
    return (yq * torch.pow(2.0, e)).reshape(x.shape)
