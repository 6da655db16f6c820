"""numpy restatement of the weight-average kernels (include/orv_mi355.h ``orv_ema_update`` / ``orv_ema_swap_in``), written from the rule and
not from the kernels.  It DEFINES them: the GPU tests demand equal bits.

    theta = the fp32 whose pattern is (p_bits << 16) + sign_extend(lo)  (32-bit wrap-around)   where low halves exist, else p_bits << 16
    s <- s - omd * (s - theta)          three fp32 operations in this order, each rounded to nearest-even on its own; omd = fp32(1 - decay)
    bf16_rne(s) = (u + 0x7fff + ((u >> 16) & 1)) >> 16 on the pattern u of s; a NaN gives (u >> 16) | 0x40

Arrays: ``s`` float32, ``p_bits`` uint16 (the bf16 patterns), ``lo`` int16 or None.  numpy keeps fp32 denormals on the CPU, as the kernels do.
``get_decay`` restates the host schedule of ``orv_amd.FusedEMA`` (``diffusers.training_utils.EMAModel``'s, from memory, unpinned)."""
import numpy as np


def omd_of(decay: float) -> np.float32:
    return np.float32(1.0 - float(decay))


def theta(p_bits, lo=None):
    u = p_bits.astype(np.uint32) << np.uint32(16)
    if lo is not None:
        u = u + lo.astype(np.int32).astype(np.uint32)            # modulo 2^32
    return u.view(np.float32)


def update(s, p_bits, lo, omd):
    """One step of the rule -> the new shadow (float32 array)."""
    s = np.asarray(s, dtype=np.float32)
    omd = np.float32(omd)
    with np.errstate(all="ignore"):
        d = (s - theta(p_bits, lo)).astype(np.float32)
        t = (omd * d).astype(np.float32)
        return (s - t).astype(np.float32)


def bf16_rne(s):
    """float32 array -> uint16 bf16 patterns."""
    u = np.asarray(s, dtype=np.float32).view(np.uint32)
    nan = (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    r = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)
    return np.where(nan, (u >> np.uint32(16)) | np.uint32(0x40), r).astype(np.uint16)


def get_decay(optimization_step, decay=0.9999, min_decay=0.0, update_after_step=0, use_ema_warmup=False, inv_gamma=1.0, power=2 / 3):
    step = max(0, optimization_step - update_after_step - 1)
    if step <= 0:
        return 0.0
    value = 1.0 - (1.0 + step / inv_gamma) ** -power if use_ema_warmup else (1.0 + step) / (10.0 + step)
    return max(min(value, decay), min_decay)


# ---- torch <-> numpy plumbing for the tests ----
def bits_of_bf16(t):
    """bf16 torch tensor (any device) -> flat uint16 numpy array of its patterns."""
    import torch
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16).reshape(-1)


def bf16_of_bits(h):
    import torch
    return torch.from_numpy(np.ascontiguousarray(h).view(np.int16).copy()).view(torch.bfloat16)
