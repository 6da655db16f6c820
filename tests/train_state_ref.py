"""numpy restatement of the checksum contract of orv_amd.train_state, and helpers the host and GPU tests share.

The contract, all arithmetic mod 2^64: pad the buffer's bytes with zero bytes to a multiple of 4, read them as little-endian u32 words
w_0 .. w_{W-1};  s1 = sum w_i;  s2 = sum (i + 1) w_i.  An empty buffer gives (0, 0)."""
import json
import os
import struct

import numpy as np
import torch

M64 = (1 << 64) - 1


def checksum_bytes(b: bytes):
    """(s1, s2) of a byte string.  numpy's uint64 sums and products wrap, which is the contract's arithmetic."""
    b = bytes(b)
    w = np.frombuffer(b + b"\0" * (-len(b) % 4), dtype="<u4").astype(np.uint64)
    if w.size == 0:
        return 0, 0
    i1 = np.arange(1, w.size + 1, dtype=np.uint64)
    with np.errstate(over="ignore"):
        return int(w.sum(dtype=np.uint64)), int((i1 * w).sum(dtype=np.uint64))


def checksum_exact(b: bytes):
    """The same pair in Python integers of unbounded size, reduced at the end: the arithmetic the numpy form must agree with."""
    b = bytes(b) + b"\0" * (-len(b) % 4)
    words = struct.unpack("<%dI" % (len(b) // 4), b)
    return sum(words) & M64, sum((i + 1) * w for i, w in enumerate(words)) & M64


def tensor_bytes(t: torch.Tensor) -> bytes:
    t = t.detach().cpu().contiguous()
    return t.view(torch.uint8).numpy().tobytes() if t.numel() else b""


def checksum(t: torch.Tensor):
    return checksum_bytes(tensor_bytes(t))


def tree_bytes(root):
    """{relative path: file bytes} of a directory tree."""
    out = {}
    for base, _, names in os.walk(root):
        for n in names:
            p = os.path.join(base, n)
            with open(p, "rb") as f:
                out[os.path.relpath(p, root)] = f.read()
    return out


def flip_byte_of(path, tensor_name, at=0):
    """Flip one bit of byte ``at`` of the named tensor's data inside a safetensors file."""
    with open(path, "rb") as f:
        raw = bytearray(f.read())
    n = struct.unpack("<Q", raw[:8])[0]
    begin, end = json.loads(raw[8:8 + n])[tensor_name]["data_offsets"]
    assert begin + at < end
    raw[8 + n + begin + at] ^= 0x10
    with open(path, "wb") as f:
        f.write(raw)


def reference_rotation(before, new, total_limit):
    """The directory names the reference's loop leaves (train_cogvideox_control_to_video_sft.py:1117-1139): before saving ``new`` it
    removes the oldest of the existing ``checkpoint-N`` so that at most ``total_limit - 1`` remain, then saves."""
    names = sorted(before, key=lambda x: int(x.split("-")[1]))
    if total_limit is not None and len(names) >= total_limit:
        names = names[len(names) - total_limit + 1:]
    return sorted(names + [new], key=lambda x: int(x.split("-")[1]))
