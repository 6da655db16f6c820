"""CPU restatement of the parameter-precision modes of the flat fused AdamW (include/orv_mi355.h ``orv_adamw_flat_ex``), written from the
rule and not from the kernels.

Split fp32 master (``split`` / ``rebuild``): the master is the fp32 value with bit pattern ``(p_bits << 16) + sign_extend(lo)`` in 32-bit
integer arithmetic; ``p_bits = (master_bits + 0x8000) >> 16`` (nearest, ties away from zero), ``lo = master_bits - (p_bits << 16)``, which
always fits int16.  A non-finite master gives the matching non-finite bf16 (NaN quiet) and ``lo = 0``.

Stochastic rounding (``sr_offsets`` / ``stochastic_round``): ``p_bits = (bits + r) >> 16`` with, modulo 2^32,
    mix(x): x ^= x >> 16 ; x *= 0x7feb352d ; x ^= x >> 15 ; x *= 0x846ca68b ; x ^= x >> 16
    key = mix(hi32(i) + mix(step + mix(seed))) ;  r(i) = mix(lo32(i) ^ key) >> 16
for the flat element index i.  Non-finite values are not perturbed; a finite value that r would carry into infinity becomes the largest
finite bf16.

``formula`` is the update itself in a chosen dtype (fp32: every operation rounded separately, in the kernel's order; float64: the yardstick),
``adamw_flat_ex`` a stand-in with the signature of ``orv_amd.ops.adamw_flat_ex`` for CPU tests of the optimizer's host logic."""
import numpy as np
import torch

MODES = {"bf16": 0, "split_fp32": 1, "stochastic": 2}


# ---- bit patterns (int64 holding the unsigned 32-bit pattern: no signed wrap-around to think about) ----
def f32_bits(x: torch.Tensor) -> torch.Tensor:
    return x.detach().cpu().contiguous().float().view(torch.int32).to(torch.int64) & 0xFFFFFFFF


def bits_f32(u: torch.Tensor) -> torch.Tensor:
    u = u & 0xFFFFFFFF
    return torch.where(u >= 2 ** 31, u - 2 ** 32, u).to(torch.int32).view(torch.float32)


def bf16_bits(p: torch.Tensor) -> torch.Tensor:
    return p.detach().cpu().contiguous().view(torch.int16).to(torch.int64) & 0xFFFF


def bits_bf16(h: torch.Tensor) -> torch.Tensor:
    h = h & 0xFFFF
    return torch.where(h >= 2 ** 15, h - 2 ** 16, h).to(torch.int16).view(torch.bfloat16)


def _nonfinite_bf16(u):
    a = u & 0x7FFFFFFF
    return (u >> 16) | torch.where(a > 0x7F800000, 0x40, 0)


def split(master: torch.Tensor):
    """fp32 -> (p bf16, lo int16)."""
    u = f32_bits(master)
    finite = (u & 0x7FFFFFFF) < 0x7F800000
    pb = torch.where(finite, ((u + 0x8000) & 0xFFFFFFFF) >> 16, _nonfinite_bf16(u))
    lo = torch.where(finite, u - (pb << 16), torch.zeros_like(u))
    assert int(lo.min()) >= -32768 and int(lo.max()) <= 32767
    return bits_bf16(pb).view(master.shape), lo.to(torch.int16).view(master.shape)


def rebuild(p: torch.Tensor, lo: torch.Tensor) -> torch.Tensor:
    """(p bf16, lo int16) -> fp32 master."""
    return bits_f32((bf16_bits(p) << 16) + lo.detach().cpu().to(torch.int64)).view(p.shape)


# ---- the counter-based hash of the stochastic mode ----
def mix32(x):
    x = np.asarray(x, dtype=np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7FEB352D)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846CA68B)
    x ^= x >> np.uint32(16)
    return x


def sr_offsets(seed: int, step: int, index) -> torch.Tensor:
    """r(i) in [0, 65535] for flat element indices ``index`` (any integer array-like), int64 tensor."""
    idx = np.asarray(index, dtype=np.uint64)
    with np.errstate(over="ignore"):
        k = mix32(np.uint32(step & 0xFFFFFFFF) + mix32(np.uint32(seed & 0xFFFFFFFF)))
        key = mix32((idx >> np.uint64(32)).astype(np.uint32) + k)
        r = mix32((idx & np.uint64(0xFFFFFFFF)).astype(np.uint32) ^ key) >> np.uint32(16)
    return torch.from_numpy(r.astype(np.int64))


def stochastic_round(x: torch.Tensor, r: torch.Tensor) -> torch.Tensor:
    """fp32 -> bf16 with the 16-bit offsets r."""
    u = f32_bits(x).view(-1)
    finite = (u & 0x7FFFFFFF) < 0x7F800000
    t = (u + r.view(-1)) & 0xFFFFFFFF
    over = (t & 0x7FFFFFFF) >= 0x7F800000
    pb = torch.where(over, ((u >> 16) & 0x8000) | 0x7F7F, t >> 16)
    return bits_bf16(torch.where(finite, pb, _nonfinite_bf16(u))).view(x.shape)


# ---- the update ----
def formula(w, g, m, v, clip, lr, beta1, beta2, eps, weight_decay, step, dtype):
    """One AdamW update of the kernel's formula, evaluated in ``dtype`` with the kernel's operation order:
        gr = g clip ; m = b1 m + (1 - b1) gr ; v = b2 v + ((1 - b2) gr) gr ; w = w (1 - lr wd) - (lr (m / bc1 as m * (1 / bc1))) / (sqrt(v (1 / bc2)) + eps)
    The hyper-parameters are first rounded to fp32 (the C ABI takes floats), so fp32 and float64 evaluations start from the same inputs.
    -> (w, m, v) in ``dtype``."""
    c = lambda x: torch.tensor(float(x), dtype=torch.float32).to(dtype)
    lr, b1, b2, eps, wd, clip, st = c(lr), c(beta1), c(beta2), c(eps), c(weight_decay), c(clip), c(step)
    one = torch.ones((), dtype=dtype)
    ibc1, ibc2 = one / (one - torch.pow(b1, st)), one / (one - torch.pow(b2, st))
    decay = one - lr * wd
    w, g, m, v = w.to(dtype), g.to(dtype), m.to(dtype), v.to(dtype)
    gr = g * clip
    m = b1 * m + (one - b1) * gr
    v = b2 * v + ((one - b2) * gr) * gr
    w = w * decay - (lr * (m * ibc1)) / (torch.sqrt(v * ibc2) + eps)
    return w, m, v


def flat_update(w, g, m, v, seg_start, seg_active, seg_step, clip, lr, beta1, beta2, eps, weight_decay, step, dtype):
    """``formula`` over a flat buffer: inactive segments keep (w, m, v); each segment uses its own step count (``seg_step`` None: ``step``)."""
    w2, m2, v2 = w.to(dtype).clone(), m.to(dtype).clone(), v.to(dtype).clone()
    starts = [int(s) for s in seg_start.tolist()]
    for i in range(len(starts) - 1):
        if not int(seg_active[i]):
            continue
        a, b = starts[i], starts[i + 1]
        st = int(seg_step[i]) if seg_step is not None else step
        w2[a:b], m2[a:b], v2[a:b] = formula(w[a:b], g[a:b], m[a:b], v[a:b], clip, lr, beta1, beta2, eps, weight_decay, st, dtype)
    return w2, m2, v2


def adamw_flat_ex(p, g, m, v, seg_start, seg_active, lr, beta1, beta2, eps, weight_decay, step, clip_coef=None, seg_step=None, lo=None,
                  mode=0, seed=0):
    """Stand-in for ``orv_amd.ops.adamw_flat_ex`` on CPU tensors (fp32 arithmetic), in place."""
    mode = MODES.get(mode, mode)
    assert mode in (0, 1, 2) and (mode != 1 or lo is not None)
    n = p.numel()
    clip = float(clip_coef) if clip_coef is not None else 1.0
    w = rebuild(p, lo) if mode == 1 else p.float()
    w2, m2, v2 = flat_update(w, g[:n].float(), m, v, seg_start, seg_active, seg_step, clip, lr, beta1, beta2, eps, weight_decay, step,
                             torch.float32)
    act = torch.zeros(n, dtype=torch.bool)
    starts = seg_start.tolist()
    for i in range(len(starts) - 1):
        act[starts[i]:starts[i + 1]] = bool(int(seg_active[i]))
    if mode == 1:
        np_, nl = split(w2)
        lo.copy_(torch.where(act, nl, lo))
    elif mode == 2:
        np_ = stochastic_round(w2, sr_offsets(seed, step, np.arange(n)))
    else:
        np_ = w2.to(torch.bfloat16)
    p.copy_(torch.where(act, np_, p))
    m.copy_(m2)
    v.copy_(v2)


def fp32_ulp(x: torch.Tensor) -> torch.Tensor:
    """The fp32 step at |x| (float64 tensor): 2^(e - 23) for |x| in [2^e, 2^(e+1)), 2^-149 below the normal range."""
    _, e = torch.frexp(x.double().abs())           # |x| = f 2^e, f in [0.5, 1)
    return torch.pow(2.0, (e - 24).clamp(min=-149).double())
