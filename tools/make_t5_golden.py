#!/usr/bin/env python
"""Writes tests/golden/t5_tiny.safetensors: the expected output of transformers' own ``T5EncoderModel`` (fp32, CPU, eval mode, no
attention mask) on a tiny T5 v1.1 encoder - d_model 128, 2 heads x 64, d_ff 128, 2 layers, vocab 64 - for one [2, 40] id tensor.

Contents (data only): ``w.<transformers key>`` the weights (bf16; they are generated bf16-representable by tests/t5_ref.make_state, so
the file is exact), ``input_ids`` int64 [2, 40], ``output`` fp32 [2, 40, 128]; the config (transformers' field names) and the key order
of ``state_dict()`` travel as JSON in the file's metadata.  Needs ``transformers``; the tests do not."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import t5_ref  # noqa: E402


def main():
    from safetensors.torch import save_file
    from transformers import T5Config, T5EncoderModel
    cfg = t5_ref.tiny_config(d_model=128, num_heads=2, d_ff=128, num_layers=2, vocab_size=64)
    state = t5_ref.make_state(cfg, seed=0)
    ids = t5_ref.make_ids(cfg, 2, 40, seed=1)
    model = T5EncoderModel(T5Config(**cfg)).float().eval()
    keys = list(model.state_dict())
    missing, unexpected = model.load_state_dict(state, strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    with torch.no_grad():
        out = model(input_ids=ids).last_hidden_state
    err = t5_ref.rel_l2(t5_ref.encode(state, cfg, ids), out)
    print(f"restatement vs transformers: rel-L2 {err:.3e}, max |out| {out.abs().max().item():.3f}")
    tensors = {"w." + k: state[k].bfloat16().contiguous().clone() for k in keys}
    tensors["input_ids"], tensors["output"] = ids.contiguous(), out.float().contiguous()
    path = os.path.join(ROOT, "tests", "golden", "t5_tiny.safetensors")
    save_file(tensors, path, metadata={"config": json.dumps(cfg), "keys": json.dumps(keys)})
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
