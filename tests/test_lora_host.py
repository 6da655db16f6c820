"""LoRA adapters, host side (no GPU): the add / save / load / fuse surface of CogVideoXTransformer3DModelTraj and the C ABI of the skinny
transposed GEMM (argument validation happens before any launch)."""
import ctypes
import json
import math
import os
import re

import pytest
import torch

import lora_ref
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def gold():
    return load_golden("fwd_actions")


def _model(gold):
    from orv_amd.cogvideox_control import CogVideoXTransformer3DModelTraj
    cfg, extra, ins, w, _ = gold
    return lora_ref.build_model(CogVideoXTransformer3DModelTraj, cfg, extra, ins, w)


def test_add_adapter_shapes_init_and_trainable_set(gold):
    m = _model(gold)
    base_ids = {id(p) for p in m.parameters()}
    m.add_adapter({"r": 8, "lora_alpha": 16})
    D = m.inner_dim
    sd = m.get_adapter_state_dict("default")
    names = lora_ref.module_names(len(m.transformer_blocks))
    assert sorted(sd) == sorted(f"{n}.lora_{ab}.weight" for n in names for ab in "AB")
    bound = 1.0 / math.sqrt(D)            # kaiming_uniform_(a = sqrt 5) on fan_in = D: U(-1 / sqrt D, 1 / sqrt D)
    for n in names:
        A, B = sd[f"{n}.lora_A.weight"], sd[f"{n}.lora_B.weight"]
        assert tuple(A.shape) == (8, D) and tuple(B.shape) == (D, 8) and A.dtype == BF16 and B.dtype == BF16
        assert torch.count_nonzero(B) == 0
        assert A.float().abs().max() <= bound * (1 + 2 ** -8) and A.float().std() > 0.3 * bound
    trainable = [p for p in m.parameters() if p.requires_grad]
    assert len(trainable) == len(sd) and all(id(p) not in base_ids for p in trainable)
    assert {p.data_ptr() for p in trainable} == {v.data_ptr() for v in sd.values()}
    assert all(not p.requires_grad for p in m.parameters() if id(p) in base_ids)
    assert m.active_adapter == "default"


def test_add_adapter_accepts_object_and_keywords_and_default_alpha(gold):
    class Cfg:
        r, lora_alpha, target_modules, init_lora_weights, use_rslora, lora_dropout, use_dora = 4, 12, ["to_q", "to_v"], True, True, 0.0, False
    m = _model(gold)
    m.add_adapter(Cfg(), adapter_name="a")
    ad = m._lora_adapters["a"]
    assert (ad.r, ad.lora_alpha, ad.use_rslora, ad.targets) == (4, 12.0, True, ["to_q", "to_v"])
    assert ad.coefficient(0.5) == pytest.approx(0.5 * 12 / 2.0)
    m.add_adapter(r=16, adapter_name="b")
    assert m._lora_adapters["b"].lora_alpha == 16.0 and m.active_adapter == "b"
    assert all(p.requires_grad for ab in m._lora_adapters["b"].params.values() for p in ab)
    assert not any(p.requires_grad for ab in m._lora_adapters["a"].params.values() for p in ab)


@pytest.mark.parametrize("kw,needle", [
    (dict(r=0), "r=0"), (dict(r=129), "r=129"),
    (dict(r=8, target_modules=["ff.net.0.proj"]), "FeedForward"),
    (dict(r=8, target_modules=["mv_blocks.0.attn1.to_q"]), "mv_blocks"),
    (dict(r=8, lora_dropout=0.1), "lora_dropout"),
    (dict(r=8, use_dora=True), "DoRA"),
])
def test_out_of_scope_configs_are_refused_with_what_is_supported(gold, kw, needle):
    m = _model(gold)
    with pytest.raises(ValueError) as e:
        m.add_adapter(**kw)
    assert needle in str(e.value) and "to_q" in str(e.value) and "to_out.0" in str(e.value)
    assert m.active_adapter is None and all(p.requires_grad for p in m.parameters())


def test_more_than_one_active_adapter_is_refused(gold):
    m = _model(gold)
    frozen = m.transformer_blocks[0].attn1.to_q.bias.requires_grad_(False)
    m.add_adapter(r=4, adapter_name="a")
    m.add_adapter(r=4, adapter_name="b")
    with pytest.raises(ValueError, match="one active adapter"):
        m.set_adapter(["a", "b"])
    m.set_adapter("a")
    assert m.active_adapter == "a"
    m.delete_adapter("a")
    assert m.active_adapter == "b"
    m.delete_adapter("b")
    assert m.active_adapter is None and not hasattr(m, "_lora_store")
    # the last delete_adapter gives back the requires_grad flags from before the first add_adapter
    assert not frozen.requires_grad and all(p.requires_grad for p in m.parameters() if p is not frozen)


def _randomise(m, name="default", seed=0):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for A, B in m._lora_adapters[name].params.values():
            A.copy_((0.1 * torch.randn(A.shape, generator=g)).to(BF16))
            B.copy_((0.1 * torch.randn(B.shape, generator=g)).to(BF16))


def test_save_load_round_trip(gold, tmp_path):
    from safetensors import safe_open
    m = _model(gold)
    m.add_adapter(r=8, lora_alpha=24, use_rslora=True)
    _randomise(m)
    path = m.save_lora_adapter(str(tmp_path))
    assert os.path.basename(path) == "pytorch_lora_weights.safetensors"
    with safe_open(path, framework="pt") as f:
        keys, meta = sorted(f.keys()), f.metadata()
    pat = re.compile(r"^transformer\.transformer_blocks\.\d+\.attn1\.(to_q|to_k|to_v|to_out\.0)\.lora_(A|B)\.weight$")
    assert len(keys) == 2 * 4 * len(m.transformer_blocks) and all(pat.match(k) for k in keys)
    md = json.loads(meta["lora_adapter_metadata"])
    assert (md["r"], md["lora_alpha"], md["use_rslora"]) == (8, 24.0, True)
    want = m.get_adapter_state_dict()
    m2 = _model(gold)
    m2.load_lora_adapter(str(tmp_path))                       # with the prefix, from the directory
    got = m2.get_adapter_state_dict()
    assert list(got) == list(want) and all(torch.equal(got[k], want[k]) for k in want)
    ad = m2._lora_adapters["default"]
    assert (ad.r, ad.lora_alpha, ad.use_rslora) == (8, 24.0, True)
    m3 = _model(gold)
    m3.load_lora_adapter({k: v.clone() for k, v in want.items()}, adapter_name="x")      # without the prefix, no metadata
    got = m3.get_adapter_state_dict("x")
    assert all(torch.equal(got[k], want[k]) for k in want)
    assert m3._lora_adapters["x"].lora_alpha == 8.0 and not m3._lora_adapters["x"].use_rslora      # alpha defaults to the rank
    m4 = _model(gold)
    sd = {"transformer." + k: v for k, v in want.items()}
    sd.update({"transformer." + n + ".alpha": torch.tensor(4.0) for n in lora_ref.module_names(len(m.transformer_blocks))})
    m4.load_lora_adapter(sd)
    assert m4._lora_adapters["default"].lora_alpha == 4.0                                           # per-module alpha scalars
    # loading into the existing adapter copies in place: same Parameter objects, bumped versions
    p0 = m2._lora_adapters["default"].params["transformer_blocks.0.attn1.to_q"][1]
    v0 = p0._version
    m2.load_lora_adapter(str(tmp_path))
    assert m2._lora_adapters["default"].params["transformer_blocks.0.attn1.to_q"][1] is p0 and p0._version > v0


def test_load_refuses_unknown_modules(gold):
    m = _model(gold)
    m.add_adapter(r=8)
    sd = {"transformer." + k: v for k, v in m.get_adapter_state_dict().items()}
    bad = dict(sd)
    bad["transformer.transformer_blocks.0.ff.net.2.lora_A.weight"] = torch.zeros(8, 512, dtype=BF16)
    bad["transformer.transformer_blocks.0.ff.net.2.lora_B.weight"] = torch.zeros(128, 8, dtype=BF16)
    with pytest.raises(ValueError, match="ff.net.2"):
        _model(gold).load_lora_adapter(bad)
    with pytest.raises(ValueError, match="unexpected key"):
        _model(gold).load_lora_adapter({**sd, "transformer.transformer_blocks.0.attn1.to_q.weight": torch.zeros(2, 2)})


def test_pipeline_save_and_load_lora_weights(gold, tmp_path):
    from orv_amd.cogvideox_control import CogVideoXImageToVideoPipelineTraj as Pipe
    m = _model(gold)
    m.add_adapter(r=8, lora_alpha=16)
    _randomise(m)
    Pipe.save_lora_weights(str(tmp_path), transformer_lora_layers=m.get_adapter_state_dict(),
                           transformer_lora_adapter_metadata={"r": 8, "lora_alpha": 16, "use_rslora": False})
    pipe = Pipe(transformer=_model(gold))
    pipe.load_lora_weights(str(tmp_path), adapter_name="robot")
    tr = pipe.transformer
    assert tr.active_adapter == "robot" and tr._lora_adapters["robot"].lora_alpha == 16.0
    want, got = m.get_adapter_state_dict(), tr.get_adapter_state_dict("robot")
    assert all(torch.equal(got[k], want[k]) for k in want)
    w0 = tr.transformer_blocks[1].attn1.to_v.weight.clone()
    pipe.fuse_lora(lora_scale=0.5)
    assert not torch.equal(tr.transformer_blocks[1].attn1.to_v.weight, w0)
    pipe.unfuse_lora()
    assert torch.equal(tr.transformer_blocks[1].attn1.to_v.weight, w0)
    pipe.unload_lora_weights()
    assert tr.active_adapter is None


def test_fuse_within_one_bf16_step_and_unfuse_exact(gold):
    m = _model(gold)
    m.add_adapter(r=8, lora_alpha=16)
    _randomise(m, seed=3)
    ad = m._lora_adapters["default"]
    orig = {k: v.clone() for k, v in m.state_dict().items()}
    c = ad.coefficient(0.75)
    m.fuse_lora(lora_scale=0.75)
    for name, (A, B) in ad.params.items():
        w = m.state_dict()[name + ".weight"]
        ref = orig[name + ".weight"].double() + c * (B.double() @ A.double())
        # one bf16 step at the reference's magnitude: spacing 2^(e - 7) for |ref| in [2^e, 2^(e + 1))
        step = torch.pow(2.0, torch.floor(torch.log2(ref.abs().clamp_min(1e-30))) - 7)
        assert ((w.double() - ref).abs() <= step).all(), name
        assert not torch.equal(w, orig[name + ".weight"])
    with pytest.raises(RuntimeError, match="fused"):
        m.add_adapter(r=4, adapter_name="other")
    m.unfuse_lora()
    now = m.state_dict()
    assert list(now) == list(orig) and all(torch.equal(now[k], orig[k]) for k in orig)


def test_state_dict_and_save_pretrained_carry_no_adapter_tensors(gold, tmp_path):
    from orv_amd.checkpoint import load_state_dict_dir
    base = _model(gold)
    base.save_pretrained(str(tmp_path / "base"))
    m = _model(gold)
    m.add_adapter(r=8)
    _randomise(m)
    assert list(m.state_dict()) == list(base.state_dict())
    m.save_pretrained(str(tmp_path / "adapted"))
    a, b = load_state_dict_dir(str(tmp_path / "adapted")), load_state_dict_dir(str(tmp_path / "base"))
    assert sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) for k in b)
    m.load_state_dict(base.state_dict(), strict=True)         # the adapter tensors are neither missing nor unexpected keys


# ---- C ABI ----
def _declared():
    with open(os.path.join(ROOT, "include", "orv_mi355.h"), "r", encoding="utf-8") as f:
        return f.read()


def test_skinny_gemm_is_declared_exported_and_bound():
    from orv_amd import _lib, ops
    hdr = _declared()
    for name in ("orv_gemm_tn_skinny_scratch", "orv_gemm_tn_skinny_bf16"):
        assert re.search(r"\b" + name + r"\(", hdr), name
        assert name in _lib.SIGNATURES
        assert getattr(_lib.lib(), name) is not None
    assert "train_cogvideox_control_to_video_sft.py:1093" in hdr[hdr.index("orv_gemm_tn_skinny_bf16") - 1500:hdr.index("orv_gemm_tn_skinny_bf16")]
    assert callable(ops.gemm_tn_skinny) and callable(ops.gemm_tn_skinny_scratch)


def test_skinny_scratch_depends_on_the_shape_only():
    from orv_amd._lib import lib
    f = lib().orv_gemm_tn_skinny_scratch
    for M, P, Q in [(1, 16, 128), (666, 64, 192), (12904, 64, 1920), (12904, 1920, 128)]:
        n = f(M, P, Q)
        assert n == f(M, P, Q) and n >= P * Q * 4 and n % (P * Q * 4) == 0
    assert f(12904, 64, 1920) == f(12904, 1920, 64)


@pytest.mark.parametrize("args,needle", [
    (dict(P=256, Q=1920), "min(P, Q)"),
    (dict(P=24), "P=24"),
    (dict(ldu=68), "ldu"),
    (dict(ldv=1924), "ldv"),
    (dict(ldc=1924), "ldc"),
    (dict(scratch=None), "scratch"),
])
def test_skinny_gemm_validates_before_any_launch(args, needle):
    """Invalid arguments come back nonzero with the offending name in orv_last_error(), without a GPU (the pointers are never followed)."""
    from orv_amd._lib import lib
    a = dict(U=4096, ldu=64, V=8192, ldv=1920, C=16384, ldc=1920, M=100, P=64, Q=1920, alpha=1.0, accumulate=0, scratch=32768)
    a.update(args)
    if "P" in args and "ldu" not in args:
        a["ldu"] = max(a["ldu"], (a["P"] + 7) // 8 * 8)
    rc = lib().orv_gemm_tn_skinny_bf16(a["U"], a["ldu"], a["V"], a["ldv"], a["C"], a["ldc"], a["M"], a["P"], a["Q"],
                                       ctypes.c_float(a["alpha"]), a["accumulate"], a["scratch"], None)
    msg = lib().orv_last_error().decode()
    assert rc != 0 and needle in msg and msg.startswith("orv_gemm_tn_skinny_bf16"), (rc, msg)
