"""MXFP8 inference mode, host side (no GPU): the C entry points are exported, ``enable_mxfp8`` toggles, a training-mode forward refuses
the mode, and the CPU restatement of the format (tests/mxfp8_ref.py) agrees with a hand-written known-answer table."""
import os
import re

import pytest
import torch

import mxfp8_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("orv_mxfp8_quantize", "orv_gemm_mxfp8", "orv_layernorm_modulate_mxfp8")


def test_library_exports_the_mxfp8_entry_points():
    from orv_amd import _lib
    header = open(os.path.join(ROOT, "include", "orv_mi355.h")).read()
    handle = _lib.lib()
    for name in NEW:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(handle, name), name


def _tiny_model():
    from conftest import load_golden
    from orv_amd.cogvideox_control import CogVideoXTransformer3DModelTraj
    cfg, extra, ins, w, outs = load_golden("fwd_actions")
    m = CogVideoXTransformer3DModelTraj(**cfg)
    m.load_state_dict(w, strict=True)
    return m, ins


def test_enable_mxfp8_toggles():
    m, _ = _tiny_model()
    assert m.mxfp8_enabled is False
    assert m.enable_mxfp8() is m and m.mxfp8_enabled is True
    assert m.enable_mxfp8(False) is m and m.mxfp8_enabled is False
    m.enable_mxfp8(True)
    assert m.mxfp8_enabled


def test_training_forward_with_mxfp8_raises():
    m, ins = _tiny_model()
    m.enable_mxfp8()
    args = (ins["hidden_states"], ins["encoder_hidden_states"], {"actions": ins["actions"]}, ins["timestep"])
    m.train()
    with pytest.raises(RuntimeError, match="MXFP8 mode is inference-only"):
        m(*args)
    m.eval()                                           # eval mode, but the forward would record gradients
    with pytest.raises(RuntimeError, match="MXFP8 mode is inference-only"):
        m(*args)
    m.enable_mxfp8(False)                              # the bf16 path's own check (no GPU here) is back
    with pytest.raises(RuntimeError, match="MI355X only"):
        with torch.no_grad():
            m(*args)


_MAXBF = torch.tensor(0x7F7F, dtype=torch.int16).view(torch.bfloat16).item()
# (block values, first 8 element bytes, scale byte): hand-derived from the rule in include/orv_mi355.h
KAT = [
    ([0.0] * 32, [0x00] * 8, 0x7F),                                                        # all-zero block: 2^0
    ([-0.0] + [0.0] * 31, [0x80] + [0x00] * 7, 0x7F),                                      # -0 stays -0
    ([448.0, 1.0, -2.0, 0.5, 0.001, 2 ** -10, 3 * 2 ** -10, -0.0] + [0.0] * 24,           # amax = 448 exactly: e = 0
     [0x7E, 0x38, 0xC0, 0x30, 0x01, 0x00, 0x02, 0x80], 0x7F),                              # e4m3 subnormals, ties to even
    ([450.0] + [0.0] * 31, [0x76] + [0x00] * 7, 0x80),                                     # just above 448: e = 1, 225 -> 224
    ([1792.0, -3.0] + [0.0] * 30, [0x7E, 0xB4] + [0x00] * 6, 0x81),                        # 448 * 2^2 exactly: e = 2; -0.75
    ([1800.0] + [0.0] * 31, [0x76] + [0x00] * 7, 0x82),                                    # just above 448 * 2^2: e = 3
    ([1.0] + [0.0] * 31, [0x78] + [0x00] * 7, 0x77),                                       # e = -8: 1 -> 256
    ([_MAXBF, -_MAXBF] + [0.0] * 30, [0x78, 0xF8] + [0x00] * 6, 0xF7),                     # +-max bf16: e = 120, 255.5 -> 256
    ([2.0 ** -130] + [0.0] * 31, [0x20] + [0x00] * 7, 0x00),                               # e clamped to -127
]


@pytest.mark.parametrize("i", range(len(KAT)))
def test_cpu_restatement_known_answers(i):
    vals, qbytes, sbyte = KAT[i]
    x = torch.tensor([vals], dtype=torch.float32)
    q, s = mxfp8_ref.quantize(x)
    assert q[0, :8].tolist() == qbytes and s.tolist() == [[sbyte]]
    # the byte form and the arithmetic form (the emulated oracle's) agree; e8m0 decodes to the scale
    assert torch.equal(mxfp8_ref.dequantize(q, s).float(), mxfp8_ref.fake_quant(x))
    assert s.view(mxfp8_ref.E8M0).float().item() == 2.0 ** (sbyte - 127)
