"""T5 text encoder, host side (no GPU): the plain-torch restatement against transformers' recorded output (and against transformers itself
when it is installed), the relative-position buckets, the module / checkpoint surface of ``orv_amd.t5.T5EncoderModel``, the C ABI of the
three T5 kernels (argument validation happens before any launch) and the pipeline's choice of the native class."""
import ctypes
import json
import os
import re
import sys

import pytest
import torch

import t5_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (d_model, heads, d_ff, layers, S, B); the second has num_heads * d_kv != d_model
CONFIGS = [(128, 2, 256, 2, 226, 2), (128, 3, 320, 4, 300, 1), (256, 4, 640, 6, 226, 2)]


@pytest.fixture(scope="module")
def tiny():
    return t5_ref.load_tiny()


def _native(cfg, state=None):
    from orv_amd.t5 import T5EncoderModel
    m = T5EncoderModel(cfg)
    if state is not None:
        m.load_state_dict(state, strict=True)
    return m


def _write_checkpoint(d, cfg, state, drop=()):
    from safetensors.torch import save_file
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "config.json"), "w", encoding="utf-8") as f:
        json.dump(cfg, f)
    save_file({k: v.bfloat16().contiguous().clone() for k, v in state.items() if k not in drop}, os.path.join(d, "model.safetensors"),
              metadata={"format": "pt"})


# ---- arithmetic of the restatement ----
def test_restatement_matches_transformers_recorded_output(tiny):
    cfg, keys, state, ids, out = tiny
    err = t5_ref.rel_l2(t5_ref.encode(state, cfg, ids), out)
    print(f"restatement vs tests/golden/t5_tiny: rel-L2 {err:.3e}")
    assert err <= 1e-5


@pytest.mark.parametrize("shape", CONFIGS, ids=lambda s: "x".join(map(str, s)))
def test_restatement_matches_transformers(shape):
    transformers = pytest.importorskip("transformers")
    D, H, F, L, S, B = shape
    cfg = t5_ref.tiny_config(d_model=D, num_heads=H, d_ff=F, num_layers=L, vocab_size=64)
    state, ids = t5_ref.make_state(cfg, seed=3), t5_ref.make_ids(cfg, B, S, seed=4)
    model = transformers.T5EncoderModel(transformers.T5Config(**cfg)).float().eval()
    missing, unexpected = model.load_state_dict(state, strict=False)
    assert not missing and not unexpected
    with torch.no_grad():
        want = model(input_ids=ids).last_hidden_state
    err = t5_ref.rel_l2(t5_ref.encode(state, cfg, ids), want)
    print(f"restatement vs transformers {shape}: rel-L2 {err:.3e}")
    assert err <= 1e-5


# ---- relative-position buckets ----
def test_bucket_known_answers():
    from orv_amd.t5 import relative_position_bucket
    rel = torch.tensor([0, 1, -1, 7, -8, 11, 12, -16, 23, -64, 90, 91, 128, -299])
    want = [0, 17, 1, 23, 8, 24, 25, 10, 27, 14, 30, 31, 31, 15]
    assert relative_position_bucket(rel).tolist() == want
    assert t5_ref.relative_position_bucket(rel).tolist() == want


def test_buckets_that_occur_over_300_positions():
    from orv_amd.t5 import relative_position_bucket
    pos = torch.arange(300)
    got = set(relative_position_bucket(pos[None, :] - pos[:, None]).flatten().tolist())
    assert got == set(range(16)) | set(range(17, 32))          # bucket 16 ("0 keys ahead") is never produced


@pytest.mark.parametrize("S", [1, 17, 300])
def test_bias_rel_builder_agrees_with_the_gathered_bias(S):
    from orv_amd.t5 import build_bias_rel
    table = torch.randn(32, 3, generator=torch.Generator().manual_seed(S))
    rel = build_bias_rel(table, S)
    assert rel.shape == (3, 2 * S - 1) and rel.dtype == torch.float32 and rel.is_contiguous()
    full = t5_ref.position_bias(table, S)                      # [H, S, S]
    i, j = torch.meshgrid(torch.arange(S), torch.arange(S), indexing="ij")
    assert torch.equal(rel[:, j - i + S - 1], full)


# ---- module / checkpoint surface ----
def test_state_dict_keys_are_transformers(tiny):
    cfg, keys, state, _, _ = tiny
    m = _native(cfg)
    assert list(m.state_dict()) == keys == t5_ref.state_keys(cfg)
    assert m.shared.weight is m.encoder.embed_tokens.weight
    assert all(not p.requires_grad for p in m.parameters()) and not m.training
    assert m.train().training is False
    assert m.config.d_model == 128 and m.config["num_heads"] == 2 and m.config.feed_forward_proj == "gated-gelu"
    m.load_state_dict(state, strict=True)
    assert m.device.type == "cpu" and m.dtype == torch.float32 and m.to(torch.bfloat16).dtype == torch.bfloat16


def test_save_load_round_trip(tiny, tmp_path):
    from orv_amd.t5 import T5EncoderModel
    cfg, keys, state, _, _ = tiny
    m = _native(cfg, state).to(torch.bfloat16)
    m.save_pretrained(str(tmp_path / "enc"))
    assert sorted(os.listdir(tmp_path / "enc")) == ["config.json", "model.safetensors"]
    back = T5EncoderModel.from_pretrained(str(tmp_path / "enc"))
    assert back.dtype == torch.bfloat16 and dict(back.config) == {**dict(m.config), "torch_dtype": "bfloat16"}
    a, b = m.state_dict(), back.state_dict()
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    assert all(torch.equal(b[k].float(), state[k]) for k in state)
    # sharded: model.safetensors.index.json + shards, through subfolder=
    m.save_pretrained(str(tmp_path / "pipe" / "text_encoder"), max_shard_size="100KB")
    names = sorted(os.listdir(tmp_path / "pipe" / "text_encoder"))
    assert "model.safetensors.index.json" in names and sum(n.startswith("model-0") for n in names) > 1
    c = T5EncoderModel.from_pretrained(str(tmp_path / "pipe"), subfolder="text_encoder", torch_dtype=torch.float32).state_dict()
    assert all(torch.equal(c[k], state[k]) for k in state)


@pytest.mark.parametrize("drop", ["shared.weight", "encoder.embed_tokens.weight"])
def test_either_embedding_key_is_enough(tiny, tmp_path, drop):
    from orv_amd.t5 import T5EncoderModel
    cfg, keys, state, _, _ = tiny
    _write_checkpoint(str(tmp_path), cfg, state, drop=(drop,))
    sd = T5EncoderModel.from_pretrained(str(tmp_path)).state_dict()
    assert torch.equal(sd["shared.weight"].float(), state["shared.weight"]) and torch.equal(sd["encoder.embed_tokens.weight"], sd["shared.weight"])


def test_decoder_keys_are_ignored_and_wrong_keys_raise(tiny, tmp_path):
    from orv_amd.t5 import T5EncoderModel
    cfg, keys, state, _, _ = tiny
    full = {**state, "decoder.block.0.layer.0.SelfAttention.q.weight": torch.zeros(128, 128), "lm_head.weight": torch.zeros(64, 128)}
    _write_checkpoint(str(tmp_path / "full"), cfg, full)
    sd = T5EncoderModel.from_pretrained(str(tmp_path / "full")).state_dict()
    assert list(sd) == keys
    _write_checkpoint(str(tmp_path / "extra"), cfg, {**state, "encoder.block.0.layer.0.SelfAttention.q.bias": torch.zeros(128)})
    with pytest.raises(RuntimeError, match="unexpected"):
        T5EncoderModel.from_pretrained(str(tmp_path / "extra"))
    _write_checkpoint(str(tmp_path / "short"), cfg, state, drop=("encoder.final_layer_norm.weight",))
    with pytest.raises(RuntimeError, match="missing"):
        T5EncoderModel.from_pretrained(str(tmp_path / "short"))


def test_unsupported_configurations_are_refused(tiny):
    from orv_amd.t5 import T5EncoderModel
    cfg = tiny[0]
    with pytest.raises(ValueError, match=r"feed_forward_proj='relu'.*supported: feed_forward_proj 'gated-gelu'"):
        T5EncoderModel({**cfg, "feed_forward_proj": "relu"})
    with pytest.raises(ValueError, match=r"d_kv=32.*supported: .*d_kv 64"):
        T5EncoderModel({**cfg, "d_kv": 32, "num_heads": 4})
    for bad in ({"d_model": 96}, {"d_ff": 100}):
        with pytest.raises(ValueError, match=r"not a multiple of 64.*supported: "):
            T5EncoderModel({**cfg, **bad})
    m = T5EncoderModel(cfg).to(torch.bfloat16)
    with pytest.raises(ValueError, match=r"must live on the GPU.*no CPU path.*supported: "):
        m(torch.zeros(1, 4, dtype=torch.long))
    with pytest.raises(ValueError, match=r"must live on the GPU"):
        m(torch.zeros(1, 4, dtype=torch.long), attention_mask=torch.ones(1, 4, dtype=torch.long))
    with pytest.raises(ValueError, match=r"masked keys are out of scope.*CogVideoX path passes none"):
        m(torch.zeros(1, 4, dtype=torch.long), attention_mask=torch.tensor([[1, 1, 1, 0]]))


def test_the_module_imports_neither_oracle_nor_transformers():
    with open(os.path.join(ROOT, "orv_amd", "t5.py"), "r", encoding="utf-8") as f:
        src = f.read()
    with open(os.path.join(ROOT, "orv_amd", "text_encoder.py"), "r", encoding="utf-8") as f:
        src += f.read()
    assert not re.search(r"^\s*(import|from)\s+(oracle|transformers)\b", src, re.M)


# ---- C ABI ----
def test_t5_symbols_are_declared_exported_and_bound():
    from orv_amd import _lib, ops
    with open(os.path.join(ROOT, "include", "orv_mi355.h"), "r", encoding="utf-8") as f:
        hdr = f.read()
    for name in ("orv_t5_attention_fwd", "orv_t5_rmsnorm", "orv_geglu", "orv_t5_attention_max_seq"):
        assert re.search(r"\b" + name + r"\(", hdr), name
        assert name in _lib.SIGNATURES
        assert getattr(_lib.lib(), name) is not None
    for name in ("orv_t5_attention_fwd", "orv_t5_rmsnorm", "orv_geglu"):
        doc = hdr[hdr.index("T5 text encoder"):hdr.index("int " + name + "(")]
        assert "orv/models/text_encoder.py:34" in doc and "cogvideox_control.py:1290-1299" in doc
    assert callable(ops.t5_attention_fwd) and callable(ops.t5_rmsnorm) and callable(ops.geglu)
    assert _lib.lib().orv_t5_attention_max_seq() >= 512
    declared = set(re.findall(r"^(?:int|long|float|size_t|const char\*)\s+(orv_\w+)\(", hdr, re.M))
    assert declared == set(_lib.SIGNATURES)                    # header symbol count == bound (and therefore exported) count


def test_t5_entry_points_validate_before_any_launch():
    """Invalid arguments come back nonzero with the reason in orv_last_error(), without a GPU (the pointers are never followed)."""
    from orv_amd._lib import lib
    h = lib()
    buf = ctypes.create_string_buffer(64)
    p = (ctypes.addressof(buf) + 15) & ~15
    err = lambda: h.orv_last_error().decode()
    smax = h.orv_t5_attention_max_seq()
    att = lambda qkv=p, ld=384, bias=p, out=p, ldo=128, B=1, S=8, H=2: h.orv_t5_attention_fwd(qkv, ld, bias, out, ldo, B, S, H, None)
    assert att(qkv=None) != 0 and "null" in err()
    assert att(S=0) != 0 and "positive" in err()
    assert att(S=smax + 1) != 0 and f"maximum of {smax}" in err() and str(smax + 1) in err()
    assert att(ld=380) != 0 and "ld_qkv" in err()
    assert att(ldo=64) != 0 and "ld_out" in err()
    assert att(qkv=p + 2) != 0 and "aligned" in err()
    rms = lambda x=p, ldx=128, w=p, y=p, ldy=128, M=4, D=128, eps=1e-6: h.orv_t5_rmsnorm(x, ldx, w, y, ldy, M, D, eps, None)
    assert rms(w=None) != 0 and "null" in err()
    assert rms(D=96) != 0 and "multiple of 64" in err()
    assert rms(ldx=64) != 0 and "ldx" in err()
    assert rms(M=0) != 0 and "M" in err()
    assert rms(eps=-1.0) != 0 and "eps" in err()
    geg = lambda hh=p, ldh=256, out=p, ldo=128, M=4, F=128: h.orv_geglu(hh, ldh, out, ldo, M, F, None)
    assert geg(out=None) != 0 and "null" in err()
    assert geg(F=100) != 0 and "multiple of 8" in err()
    assert geg(ldh=128) != 0 and "ldh" in err()
    assert geg(hh=p + 4) != 0 and "aligned" in err()
    assert all(err().startswith(n) for n, f in (("orv_geglu", geg(M=0)),))


# ---- pipeline ----
def test_pipeline_from_pretrained_picks_the_native_encoder_without_transformers(tiny, tmp_path, monkeypatch, golden):
    from orv_amd.cogvideox_control import CogVideoXImageToVideoPipelineTraj, CogVideoXTransformer3DModelTraj
    from orv_amd.schedulers import CogVideoXDDIMScheduler
    from orv_amd.t5 import T5EncoderModel
    cfg, keys, state, _, _ = tiny
    tcfg = golden("fwd_actions")[0]
    pipe = CogVideoXImageToVideoPipelineTraj(transformer=CogVideoXTransformer3DModelTraj(**tcfg), scheduler=CogVideoXDDIMScheduler(prediction_type="v_prediction"))
    pipe.save_pretrained(str(tmp_path))
    _write_checkpoint(str(tmp_path / "text_encoder"), cfg, state)
    monkeypatch.setitem(sys.modules, "transformers", None)      # `import transformers` now raises ImportError
    got = CogVideoXImageToVideoPipelineTraj.from_pretrained(str(tmp_path))
    assert isinstance(got.text_encoder, T5EncoderModel) and got.tokenizer is None
    assert all(torch.equal(v.float(), state[k]) for k, v in got.text_encoder.state_dict().items())
    with pytest.raises(NotImplementedError, match=r"orv_amd\.t5\.T5EncoderModel"):
        got._get_t5_prompt_embeds("a prompt")
    os.remove(tmp_path / "text_encoder" / "model.safetensors")  # no weights: None, as the transformers branch leaves it
    assert CogVideoXImageToVideoPipelineTraj.from_pretrained(str(tmp_path)).text_encoder is None


def test_text_encoder_helpers_take_token_ids_without_a_tokenizer():
    from orv_amd import text_encoder as te

    class Enc:
        device = torch.device("cpu")

        def __call__(self, ids):
            return (ids.float()[..., None].repeat(1, 1, 4),)

    ids = torch.arange(6).view(2, 3)
    out = te.compute_prompt_embeddings(None, Enc(), None, 3, torch.device("cpu"), torch.float32, text_input_ids=ids)
    assert torch.equal(out, Enc()(ids)[0])
    two = te.encode_prompt(None, Enc(), None, num_videos_per_prompt=2, device=torch.device("cpu"), dtype=torch.float32, text_input_ids=ids)
    assert two.shape == (4, 3, 4) and torch.equal(two[1], two[0])
    with pytest.raises(ValueError, match="text_input_ids"):
        te.encode_prompt(None, Enc(), "x")
    tok = lambda prompts, **kw: {"input_ids": torch.full((len(prompts), kw["max_length"]), 5)}
    assert te.encode_prompt(tok, Enc(), ["a", "b"], max_sequence_length=7, dtype=torch.float32).shape == (2, 7, 4)
