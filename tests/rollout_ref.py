"""numpy restatement of the two value contracts of a cascaded rollout's chunk boundary (csrc/frames.hip), and the
value sweep the host and the GPU tests share.  Checker only: nothing in the package imports this."""
import numpy as np

F32 = np.float32


def quantize_ref(x):
    """fp32 values -> uint8 levels: y = fl(fl(x / 2) + 0.5), clamp to [0, 1], rint_half_even(fl(y * 255)); NaN -> 0."""
    x = np.asarray(x, dtype=F32)
    with np.errstate(invalid="ignore"):
        y = x / F32(2)
        y = y + F32(0.5)
        y = np.minimum(np.maximum(y, F32(0)), F32(1))
        u = np.rint(y * F32(255))
    assert u.dtype == F32
    return np.where(np.isnan(x), F32(0), u).astype(np.uint8)


def quantize_frames_ref(video):
    """fp32 [B, 3, F, H, W] -> uint8 [B, F, H, W, 3]."""
    return np.ascontiguousarray(quantize_ref(video).transpose(0, 2, 3, 4, 1))


def bf16_bits(x):
    """fp32 -> the bits of the nearest bf16, ties to even (finite values)."""
    u = np.asarray(x, dtype=F32).view(np.uint32)
    return ((u + np.uint32(0x7fff) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def bf16_to_f32(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(F32)


def handoff_table_ref():
    """level -> bf16 bits of fl(2 fl(level / 255) - 1): uint16 [256]."""
    x = np.arange(256, dtype=np.uint8).astype(F32) / F32(255.0)
    return bf16_bits(F32(2.0) * x - F32(1.0))


def handoff_ref(frames, index):
    """uint8 [B, F, H, W, 3] -> the bf16 bits of the encoder's input, uint16 [B, 1, H, W, 8] (channels 3-7 zero)."""
    B, _, H, W, _ = frames.shape
    out = np.zeros((B, 1, H, W, 8), dtype=np.uint16)
    out[:, 0, :, :, :3] = handoff_table_ref()[frames[:, index]]
    return out


def halfway_inputs():
    """fp32 inputs x whose y = fl(fl(x / 2) + 0.5) gives fl(y * 255) = k + 0.5 exactly, where the rounding rule decides the level:
    -> (x, k).  y - 0.5 and the doubling are exact for y >= 0.25, so most k in [64, 254] have such an x; every candidate is verified
    forwards."""
    xs, ks = [], []
    for k in range(255):
        y0 = F32((k + 0.5) / 255.0)
        for step in range(-3, 4):
            y = y0
            for _ in range(abs(step)):
                y = np.nextafter(y, F32(2.0) if step > 0 else F32(-1.0))
            x = F32(2) * (y - F32(0.5))
            yy = x / F32(2) + F32(0.5)
            if yy * F32(255) == F32(k + 0.5):
                xs.append(x), ks.append(k)
    return np.array(xs, dtype=F32), np.array(ks)


def sweep(nan: bool = True):
    """Every bf16 value in [-1.5, 1.5] (zeros and denormals included), the half-way cases, +-inf and (optionally) a NaN: fp32 [n]."""
    vals = bf16_to_f32(np.arange(1 << 16, dtype=np.uint32).astype(np.uint16))
    vals = vals[np.isfinite(vals) & (np.abs(vals) <= F32(1.5))]
    extra = [F32(np.inf), F32(-np.inf)] + ([F32(np.nan)] if nan else [])
    return np.concatenate([vals, halfway_inputs()[0], np.array(extra, dtype=F32)])


def sweep_video(width: int = 40, nan: bool = True):
    """The sweep laid out as one fp32 clip [1, 3, 1, H, width], padded with zeros."""
    v = sweep(nan)
    H = -(-v.size // (3 * width))
    out = np.zeros(3 * H * width, dtype=F32)
    out[:v.size] = v
    return out.reshape(1, 3, 1, H, width)
