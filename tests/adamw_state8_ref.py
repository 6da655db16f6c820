"""CPU restatement of the block-scaled fp8 optimizer moments of the flat fused AdamW (include/orv_mi355.h ``orv_adamw_flat_s8``,
``orv_state8_quantize``, ``orv_state8_dequantize``; the format is defined in orv_amd/csrc/optim_s8.hip), written from the rule and not from
the kernels: exponents come from ``frexp`` and exact float64 scalings, not from fp32 bit tricks.

A block is 256 consecutive flat elements, stored as 256 element bytes and one scale byte ``e + 127``.  First moment: e4m3fn (M 3, Emin -6,
F 448); second moment: e5m2 (M 2, Emin -14, F 57344).
    e       = smallest integer with amax <= F 2^e, clamped to [-127, 127]; amax over the FINITE values of the block (none, or all zero: -127)
    y       = fp32(x 2^-e), a = |y|                                   (one fp32 product, subnormals kept)
    E       = max(floor(log2 a), Emin), s = 2^(E - M), w = floor(a / s 65536), n = (w + r) >> 16, stored magnitude n s, sign of x
    x not finite: byte 0x7F
    r       : key2 = mix(hi32(i) + mix(step + mix(seed ^ 0x9E3779B9))), h = mix(lo32(i) ^ key2), r_m = h >> 16, r_v = h & 0xFFFF
    value   = code_value 2^e                                            (exact in fp32)
    update  : the fp32 formula of ``adamw_ref.formula`` with sqrt(max(v, 2^(e_v_old - 16)) / bc2) in the denominator

``adamw_flat_s8`` / ``state8_quantize`` / ``state8_dequantize`` are stand-ins with the signatures of ``orv_amd.ops`` for CPU tests of the
optimizer's host logic."""
import numpy as np
import torch

import adamw_ref

BLOCK = 256
FORMATS = {0: dict(M=3, Emin=-6, F=448.0), 1: dict(M=2, Emin=-14, F=57344.0)}
_NAMES = {"m": 0, "v": 1}


def _fmt(fmt):
    return FORMATS[_NAMES.get(fmt, fmt)]


def _np(x, dtype=np.float32):
    """Flat array of x in ``dtype``: fp32 is the format's own input type; float64 serves the GPU tests, which ask where a float64
    evaluation of the moments would land (no rounding in the scaling product then)."""
    if torch.is_tensor(x):
        x = x.detach().cpu().contiguous().numpy()
    return np.ascontiguousarray(x, dtype=dtype).reshape(-1)


def state_offsets(seed: int, step: int, index):
    """(r_m, r_v) in [0, 65535] for flat element indices ``index``, int64 arrays."""
    idx = np.asarray(index, dtype=np.uint64)
    mix = adamw_ref.mix32
    with np.errstate(over="ignore"):
        k = mix(np.uint32(step & 0xFFFFFFFF) + mix(np.uint32((seed ^ 0x9E3779B9) & 0xFFFFFFFF)))
        key2 = mix((idx >> np.uint64(32)).astype(np.uint32) + k)
        h = mix((idx & np.uint64(0xFFFFFFFF)).astype(np.uint32) ^ key2)
    return (h >> np.uint32(16)).astype(np.int64), (h & np.uint32(0xFFFF)).astype(np.int64)


def block_exponents(x, fmt, dtype=np.float32) -> np.ndarray:
    """e per block of 256 (int64) for the values x."""
    f = _fmt(fmt)
    a = np.abs(_np(x, dtype).astype(np.float64))
    amax = np.where(np.isfinite(a), a, 0.0).reshape(-1, BLOCK).max(axis=1)
    fm, fe = np.frexp(f["F"])                       # F = fm 2^fe, fm in [0.5, 1)
    am, ae = np.frexp(amax)                         # amax = am 2^ae
    e = ae - fe + (am > fm)                         # amax <= F 2^e  <=>  am 2^(ae - fe - e) <= fm
    e = np.where(amax > 0, e, -127)
    return np.clip(e, -127, 127).astype(np.int64)


def encode(x, e, r, fmt, dtype=np.float32) -> np.ndarray:
    """Element bytes (uint8) of the values x with per-ELEMENT block exponent e and 16-bit offsets r."""
    f = _fmt(fmt)
    M, Emin = f["M"], f["Emin"]
    x = _np(x, dtype)
    e = np.asarray(e, dtype=np.int64).reshape(-1)
    r = np.asarray(r, dtype=np.int64).reshape(-1)
    with np.errstate(invalid="ignore", over="ignore"):
        y = x * np.ldexp(dtype(1.0), -e).astype(dtype)                      # one fp32 product
    finite = np.isfinite(x)
    a = np.where(finite, np.abs(y.astype(np.float64)), 0.0)
    _, ae = np.frexp(a)
    E = np.maximum(np.where(a > 0, ae - 1, Emin), Emin)
    w = np.floor(np.ldexp(a, 16 - (E - M))).astype(np.int64)                # a / s 65536, exact before the floor
    n = (w + r) >> 16
    code = np.where(n < (1 << M), n, ((E - Emin + 1) << M) + n - (1 << M))
    code = code | np.where(np.signbit(x), 0x80, 0)
    return np.where(finite, code, 0x7F).astype(np.uint8)


def code_values(q, fmt) -> np.ndarray:
    """Element bytes -> their values on the unit grid, float64 (0x7F / 0xFF: NaN; the infinity codes of e5m2 decode as in IEEE)."""
    f = _fmt(fmt)
    M, Emin = f["M"], f["Emin"]
    c = np.asarray(q.detach().cpu().numpy() if torch.is_tensor(q) else q, dtype=np.uint8).reshape(-1).astype(np.int64)
    mag, ef, mant = c & 0x7F, (c & 0x7F) >> M, c & ((1 << M) - 1)
    val = np.where(ef == 0, np.ldexp(mant.astype(np.float64), Emin - M), np.ldexp(((1 << M) + mant).astype(np.float64), ef - 1 + Emin - M))
    if M == 3:
        val = np.where(mag == 0x7F, np.nan, val)
    else:
        val = np.where(mag == 0x7C, np.inf, np.where(mag > 0x7C, np.nan, val))
    return np.where(c & 0x80, -val, val)


def quantize(x, fmt, seed=0, step=0, index0=0, r=None, dtype=np.float32):
    """fp32 values (a multiple of 256, at flat indices index0...) -> (element bytes uint8, scale bytes uint8) as torch tensors.  ``r``
    overrides the hash offsets (an int or an array)."""
    x = _np(x, dtype)
    assert x.size % BLOCK == 0
    e = block_exponents(x, fmt, dtype)
    if r is None:
        r = state_offsets(seed, step, np.arange(index0, index0 + x.size, dtype=np.uint64))[_NAMES.get(fmt, fmt)]
    r = np.broadcast_to(np.asarray(r, dtype=np.int64), (x.size,))
    q = encode(x, np.repeat(e, BLOCK), r, fmt, dtype)
    return torch.from_numpy(q), torch.from_numpy((e + 127).astype(np.uint8))


def dequantize(q, exps, fmt) -> torch.Tensor:
    """(element bytes, scale bytes) -> fp32 values (exact)."""
    e = np.repeat(np.asarray(exps.detach().cpu().numpy(), dtype=np.int64).reshape(-1) - 127, BLOCK)
    val = np.ldexp(code_values(q, fmt), e)
    out = val.astype(np.float32)
    ok = ~np.isfinite(val) | (out.astype(np.float64) == val)
    assert bool(ok.all()), "dequantisation must be exact in fp32"
    return torch.from_numpy(out)


def grid_step(q, exps, fmt) -> np.ndarray:
    """The grid step s 2^e at each stored element (float64): the distance to the next code upward in magnitude."""
    f = _fmt(fmt)
    c = np.asarray(q.detach().cpu().numpy(), dtype=np.uint8).reshape(-1).astype(np.int64)
    ef = (c & 0x7F) >> f["M"]
    e = np.repeat(np.asarray(exps.detach().cpu().numpy(), dtype=np.int64).reshape(-1) - 127, BLOCK)
    return np.ldexp(1.0, np.maximum(ef - 1, 0) + f["Emin"] - f["M"] + e)


# ---- the update ----
def formula(w, g, m, v, vfloor, clip, lr, beta1, beta2, eps, weight_decay, step, dtype):
    """``adamw_ref.formula`` with the floored second moment in the denominator (the returned v is the un-floored one)."""
    c = lambda x: torch.tensor(float(x), dtype=torch.float32).to(dtype)
    lr, b1, b2, eps, wd, clip, st = c(lr), c(beta1), c(beta2), c(eps), c(weight_decay), c(clip), c(step)
    one = torch.ones((), dtype=dtype)
    ibc1, ibc2 = one / (one - torch.pow(b1, st)), one / (one - torch.pow(b2, st))
    decay = one - lr * wd
    w, g, m, v, vfloor = w.to(dtype), g.to(dtype), m.to(dtype), v.to(dtype), vfloor.to(dtype)
    gr = g * clip
    m = b1 * m + (one - b1) * gr
    v = b2 * v + ((one - b2) * gr) * gr
    w = w * decay - (lr * (m * ibc1)) / (torch.sqrt(torch.maximum(v, vfloor) * ibc2) + eps)
    return w, m, v


def v_floor(v_exp) -> torch.Tensor:
    """2^(e_v_old - 16) per ELEMENT from the incoming second-moment scale bytes, float64."""
    e = v_exp.detach().cpu().to(torch.int64) - 127
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), (e - 16).double()).repeat_interleave(BLOCK)


def active_mask(n, seg_start, seg_active) -> torch.Tensor:
    act = torch.zeros(n, dtype=torch.bool)
    starts = [int(s) for s in seg_start.tolist()]
    for i in range(len(starts) - 1):
        act[starts[i]:starts[i + 1]] = bool(int(seg_active[i]))
    return act


def flat_update(w, g, m, v, vfloor, seg_start, seg_active, seg_step, clip, lr, beta1, beta2, eps, weight_decay, step, dtype):
    """``formula`` over a flat buffer: inactive segments keep (w, m, v); each segment uses its own step count (``seg_step`` None: ``step``)."""
    w2, m2, v2 = w.to(dtype).clone(), m.to(dtype).clone(), v.to(dtype).clone()
    starts = [int(s) for s in seg_start.tolist()]
    for i in range(len(starts) - 1):
        if not int(seg_active[i]):
            continue
        a, b = starts[i], starts[i + 1]
        st = int(seg_step[i]) if seg_step is not None else step
        w2[a:b], m2[a:b], v2[a:b] = formula(w[a:b], g[a:b], m[a:b], v[a:b], vfloor[a:b], clip, lr, beta1, beta2, eps, weight_decay, st, dtype)
    return w2, m2, v2


def store_weight(w32, p, lo, act, mode, seed, step):
    """Store the fp32 results by ``mode`` into p (and lo) where ``act``, as orv_adamw_flat_ex does (mode 0: nearest-even bf16)."""
    n = p.numel()
    if mode == 1:
        np_, nl = adamw_ref.split(w32)
        lo.copy_(torch.where(act, nl, lo))
    elif mode == 2:
        np_ = adamw_ref.stochastic_round(w32, adamw_ref.sr_offsets(seed, step, np.arange(n)))
    else:
        np_ = w32.to(torch.bfloat16)
    p.copy_(torch.where(act, np_, p))


def adamw_flat_s8(p, g, m8, v8, m_exp, v_exp, seg_start, seg_active, lr, beta1, beta2, eps, weight_decay, step, clip_coef=None,
                  seg_step=None, lo=None, mode=0, seed=0):
    """Stand-in for ``orv_amd.ops.adamw_flat_s8`` on CPU tensors (fp32 arithmetic), in place."""
    mode = adamw_ref.MODES.get(mode, mode)
    assert mode in (0, 1, 2) and (mode != 1 or lo is not None)
    n = p.numel()
    clip = float(clip_coef) if clip_coef is not None else 1.0
    w = adamw_ref.rebuild(p, lo) if mode == 1 else p.float()
    m, v = dequantize(m8, m_exp, 0), dequantize(v8, v_exp, 1)
    w2, m2, v2 = flat_update(w, g[:n].float(), m, v, v_floor(v_exp).float(), seg_start, seg_active, seg_step, clip, lr, beta1, beta2, eps,
                             weight_decay, step, torch.float32)
    act = active_mask(n, seg_start, seg_active)
    store_weight(w2, p, lo, act, mode, seed, step)
    for x2, q, ex, fmt in ((m2, m8, m_exp, 0), (v2, v8, v_exp, 1)):
        nq, ne = quantize(x2, fmt, seed, step)
        q.copy_(torch.where(act, nq, q))
        ex.copy_(torch.where(act[::BLOCK], ne, ex))


def state8_quantize(x, q, exps, fmt, seed=0, step=0):
    nq, ne = quantize(x, fmt, seed, step)
    q.copy_(nq), exps.copy_(ne)


def state8_dequantize(q, exps, x, fmt):
    x.copy_(dequantize(q, exps, fmt))
