"""GPU parity of the T5 text encoder: the three kernels through ``orv_amd.ops`` against fp32 torch at the project's per-op bar
(|err| <= 1.6e-2 |ref| + 1e-2 max|ref|), the whole ``orv_amd.t5.T5EncoderModel`` against the fp32 restatement (tests/t5_ref.py) at
1.25 x the error of the same restatement run in bf16, and ``pipe(prompt=...)`` with nothing but a tokenizer attached."""
import functools

import pytest
import torch

import t5_ref

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def q(x):
    return x.to(BF).float()


def close(got, ref, rtol=1.6e-2, afrac=1e-2):
    got, ref = got.float().cpu(), ref.float().cpu()
    assert torch.isfinite(got).all()
    atol = afrac * ref.abs().max().item() + 1e-6
    err = (got - ref).abs()
    bad = err > (rtol * ref.abs() + atol)
    print(f"max err {err.max().item():.4g}, atol {atol:.4g}, max |ref| {ref.abs().max().item():.4g}")
    assert not bad.any(), f"max err {err.max().item():.4g} vs atol {atol:.4g} ({int(bad.sum())} bad)"


# ---- attention ----
def _attn_inputs(B, S, H, seed, q_scale=1.0, bias_scale=1.0):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, S, 3, H, 64, generator=g)
    qkv[:, :, 0] *= 0.25 * q_scale                            # q . k ~ N(0, 4): score std 2, as the generated weights give
    bias_rel = torch.randn(H, 2 * S - 1, generator=g) * bias_scale
    return q(qkv), bias_rel


def _attn_ref(qkv, bias_rel):
    B, S, _, H, _ = qkv.shape
    qq, kk, vv = (qkv[:, :, i].permute(0, 2, 1, 3).double() for i in range(3))          # [B, H, S, 64]
    i, j = torch.meshgrid(torch.arange(S), torch.arange(S), indexing="ij")
    s = qq @ kk.transpose(-1, -2) + bias_rel[:, j - i + S - 1].double()
    return (torch.softmax(s, -1) @ vv).permute(0, 2, 1, 3).reshape(B * S, H * 64).float()


def _attn_run(qkv, bias_rel, dev):
    from orv_amd import ops
    B, S, _, H, _ = qkv.shape
    out = torch.full((B * S, H * 64), float("nan"), dtype=BF, device=dev)
    ops.t5_attention_fwd(qkv.reshape(B * S, 3 * H * 64).to(dev, BF), bias_rel.to(dev), out, B, S, H)
    return out


@pytest.mark.parametrize("B,S,H", [(1, 1, 1), (2, 17, 2), (1, 64, 3), (2, 226, 4), (1, 300, 2), (1, 512, 2)])
def test_t5_attention_matches_fp32(B, S, H):
    dev = torch.device("cuda:0")
    qkv, bias = _attn_inputs(B, S, H, seed=S)
    close(_attn_run(qkv, bias, dev), _attn_ref(qkv, bias))


def test_t5_attention_zero_q_is_softmax_of_the_bias():
    """q = 0: the output is softmax(bias) v; the table's +n and -n entries differ, so a transposed or mirrored lookup shows."""
    dev = torch.device("cuda:0")
    qkv, bias = _attn_inputs(1, 100, 2, seed=5)
    qkv[:, :, 0] = 0
    bias = bias + torch.linspace(-3, 3, 199)[None, :]          # strongly asymmetric in j - i
    ref = _attn_ref(qkv, bias)
    close(_attn_run(qkv, bias, dev), ref)
    assert (ref - _attn_ref(qkv, bias.flip(1))).abs().max() > 0.1 * ref.abs().max()    # the mirrored table is far outside the bar


def test_t5_attention_large_scores_and_large_bias():
    dev = torch.device("cuda:0")
    qkv, bias = _attn_inputs(2, 130, 2, seed=6, q_scale=8.0)   # |score| reaches the hundreds: only the true row maximum keeps exp finite
    out = _attn_run(qkv, bias, dev)
    assert torch.isfinite(out.float()).all()
    close(out, _attn_ref(qkv, bias))
    qkv, bias = _attn_inputs(1, 130, 2, seed=7)
    bias = torch.where(torch.rand(bias.shape, generator=torch.Generator().manual_seed(8)) < 0.5, 20.0, -20.0)
    close(_attn_run(qkv, bias, dev), _attn_ref(qkv, bias))


def test_t5_attention_is_deterministic_and_batch_invariant():
    dev = torch.device("cuda:0")
    qkv, bias = _attn_inputs(2, 226, 3, seed=9)
    both = _attn_run(qkv, bias, dev)
    assert torch.equal(both, _attn_run(qkv, bias, dev))
    singles = torch.cat([_attn_run(qkv[b:b + 1], bias, dev) for b in range(2)])
    assert torch.equal(both, singles)


def test_t5_attention_refuses_sequences_above_the_maximum():
    from orv_amd import ops
    dev = torch.device("cuda:0")
    S = ops.t5_attention_max_seq() + 1
    qkv = torch.zeros(S, 192, dtype=BF, device=dev)
    out = torch.zeros(S, 64, dtype=BF, device=dev)
    with pytest.raises(RuntimeError, match=f"maximum of {S - 1}"):
        ops.t5_attention_fwd(qkv, torch.zeros(1, 2 * S - 1, device=dev), out, 1, S, 1)


def test_t5_attention_strided_rows_leave_the_padding_alone():
    from orv_amd import ops
    dev = torch.device("cuda:0")
    B, S, H = 2, 70, 2
    qkv, bias = _attn_inputs(B, S, H, seed=10)
    ld_qkv, ld_out = 3 * H * 64 + 64, H * 64 + 24
    wide = torch.full((B * S, ld_qkv), float("nan"), dtype=BF, device=dev)           # NaN padding: reading it would poison the result
    wide[:, :3 * H * 64] = qkv.reshape(B * S, -1).to(dev, BF)
    out = torch.full((B * S + 3, ld_out), 7.0, dtype=BF, device=dev)
    ops.t5_attention_fwd(wide, bias.to(dev), out, B, S, H, ld_qkv=ld_qkv, ld_out=ld_out)
    close(out[:B * S, :H * 64], _attn_ref(qkv, bias))
    assert bool((out[:B * S, H * 64:] == 7.0).all()) and bool((out[B * S:] == 7.0).all())


# ---- RMS LayerNorm / gated GELU ----
@pytest.mark.parametrize("M,D", [(1, 128), (226, 320), (452, 4096)])
def test_t5_rmsnorm_matches_fp32(M, D):
    from orv_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(M)
    x = torch.randn(M, D, generator=g)
    x[0] *= 1e-3                                               # rows of magnitude 1e-3 and 1e3 in one call
    x[-1] *= 1e3
    x, w = q(x), q(1 + 0.1 * torch.randn(D, generator=g))
    y = torch.full((M, D), float("nan"), dtype=BF, device=dev)
    ops.t5_rmsnorm(x.to(dev, BF), w.to(dev, BF), y, M, D, 1e-6)
    close(y, t5_ref.rms(x, w, 1e-6))


@pytest.mark.parametrize("M,F", [(226, 256), (452, 10240)])
def test_geglu_matches_fp32(M, F):
    from orv_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(F)
    h = torch.randn(M, 2 * F, generator=g) * 2
    h[:, :64] = torch.linspace(-30, 30, 64)                    # gate inputs reaching +-30
    h[:, F:F + 64] = torch.linspace(30, -30, 64)
    h = q(h)
    out = torch.full((M, F), float("nan"), dtype=BF, device=dev)
    ops.geglu(h.to(dev, BF), out, M, F)
    assert not torch.isnan(out.float()).any()
    close(out, t5_ref.gelu_new(h[:, :F].double()).float() * h[:, F:])


# ---- whole encoder ----
# (d_model, heads, d_ff, layers, S, B, vocab): the three configurations of the host test and one full-width layer
ENCODERS = {"small": (128, 2, 256, 2, 226, 2, 64), "inner_ne_d": (128, 3, 320, 4, 300, 1, 64), "deep": (256, 4, 640, 6, 226, 2, 64),
            "full_width": (4096, 64, 10240, 1, 226, 2, 512)}


@functools.lru_cache(maxsize=None)
def _case(name):
    """(cfg, state, ids, fp32 restatement, yardstick): computed once per case and shared; the yardstick is the restatement in bf16
    against its own fp32 run."""
    if name == "tiny_fixture":
        cfg, _, state, ids, _ = t5_ref.load_tiny()
    else:
        D, H, F, L, S, B, V = ENCODERS[name]
        cfg = t5_ref.tiny_config(d_model=D, num_heads=H, d_ff=F, num_layers=L, vocab_size=V)
        state, ids = t5_ref.make_state(cfg, seed=3), t5_ref.make_ids(cfg, B, S, seed=4)
    with torch.no_grad():
        ref = t5_ref.encode(state, cfg, ids)
        yard = t5_ref.rel_l2(t5_ref.encode(state, cfg, ids, dtype=BF).float(), ref)
    return cfg, state, ids, ref, yard


def _encoder(cfg, state, dev):
    from orv_amd.t5 import T5EncoderModel
    m = T5EncoderModel(cfg)
    m.load_state_dict(state, strict=True)
    return m.to(dev, BF)


@pytest.mark.parametrize("name", ["small", "inner_ne_d", "deep", "full_width", "tiny_fixture"])
def test_t5_encoder_matches_the_fp32_restatement(name):
    dev = torch.device("cuda:0")
    cfg, state, ids, ref, yard = _case(name)
    enc = _encoder(cfg, state, dev)
    out = enc(ids.to(dev))
    assert out[0] is out.last_hidden_state and out[0].dtype == BF and tuple(out[0].shape) == tuple(ref.shape)
    err = t5_ref.rel_l2(out[0].float().cpu(), ref)
    print(f"[t5-err] {name}: rel-L2(HIP, fp32 restatement) = {err:.4e}, bf16 restatement yardstick = {yard:.4e}, bar = {1.25 * yard:.4e}")
    assert torch.isfinite(out[0].float()).all()
    assert err <= 1.25 * yard, (name, err, yard)
    assert torch.equal(enc(ids.to(dev))[0], out[0])            # two runs: the same bits
    assert torch.equal(enc(ids.to(dev), attention_mask=torch.ones_like(ids), return_dict=False)[0], out[0])


def test_t5_encoder_fixture_matches_transformers_recorded_output():
    dev = torch.device("cuda:0")
    cfg, _, state, ids, want = t5_ref.load_tiny()
    yard = _case("tiny_fixture")[4]
    err = t5_ref.rel_l2(_encoder(cfg, state, dev)(ids.to(dev))[0].float().cpu(), want)
    print(f"[t5-err] tiny fixture vs transformers' fp32 output: {err:.4e} (bar {1.25 * yard:.4e})")
    assert err <= 1.25 * yard


def test_t5_encoder_follows_weight_changes_and_refuses_masks():
    dev = torch.device("cuda:0")
    cfg, state, ids, ref, yard = _case("small")
    enc = _encoder(cfg, state, dev)
    ids = ids[:, :40].to(dev)
    first = enc(ids)[0].clone()
    other = t5_ref.make_state(cfg, seed=11)
    enc.load_state_dict(other, strict=True)                    # in place: the stacked q|k|v and wi_0|wi_1 operands must follow
    with torch.no_grad():
        want = t5_ref.encode(other, cfg, ids.cpu())
    got = enc(ids)[0]
    assert not torch.equal(got, first) and t5_ref.rel_l2(got.float().cpu(), want) <= 2e-2
    assert all(torch.equal(v.float().cpu(), other[k]) for k, v in enc.state_dict().items())
    mask = torch.ones_like(ids)
    mask[0, -1] = 0
    with pytest.raises(ValueError, match="masked keys are out of scope.*CogVideoX path passes none"):
        enc(ids, attention_mask=mask)
    with pytest.raises(ValueError, match="must live on the GPU"):
        enc(ids.cpu())


# ---- pipeline ----
class StubTokenizer:
    """The call shape of transformers' T5Tokenizer as the pipeline uses it; ids are a seeded function of the prompt."""

    def __init__(self, vocab):
        self.vocab = vocab

    def __call__(self, prompts, padding=None, max_length=None, truncation=None, add_special_tokens=None, return_tensors=None):
        rows = [torch.randint(0, self.vocab, (max_length,), generator=torch.Generator().manual_seed(sum(map(ord, p)))) for p in prompts]
        return {"input_ids": torch.stack(rows)}


def test_pipeline_takes_prompts_with_the_native_encoder(golden):
    from orv_amd import schedulers, text_encoder as te
    from orv_amd.cogvideox_control import CogVideoXImageToVideoPipelineTraj, CogVideoXTransformer3DModelTraj
    dev = torch.device("cuda:0")
    tcfg, extra, ins, _, _ = golden("pipe_ddim_bf16")
    cfg, _, state, _, _ = t5_ref.load_tiny()
    torch.manual_seed(0)
    tr = CogVideoXTransformer3DModelTraj(**{**tcfg, "text_embed_dim": cfg["d_model"]})
    for p in tr.parameters():
        if p.ndim >= 2:
            p.data.normal_(0, 0.05)
    tr = tr.to(dev, BF).eval()
    tr.action_embed.forced_mask = torch.zeros(2, dtype=torch.bool)
    sched = schedulers.CogVideoXDDIMScheduler(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                                              clip_sample=False, set_alpha_to_one=True, prediction_type="v_prediction",
                                              rescale_betas_zero_snr=True, snr_shift_scale=3.0, timestep_spacing="trailing")
    enc = _encoder(cfg, state, dev)
    pipe = CogVideoXImageToVideoPipelineTraj(tokenizer=StubTokenizer(cfg["vocab_size"]), text_encoder=enc, transformer=tr, scheduler=sched)
    L = tcfg["max_text_seq_length"]
    prompts, negs = ["a robot arm picks up the cup", "the gripper opens"], ["blurry, low quality"] * 2
    kw = dict(image=ins["image"].to(dev, BF), height=64, width=96, num_frames=9, num_inference_steps=2, guidance_scale=6,
              output_type="latent", controls_or_guidances={}, max_sequence_length=L)
    a = pipe(prompt=prompts, negative_prompt=negs, generator=torch.Generator().manual_seed(1), **kw).frames
    pe, ne = pipe.encode_prompt(prompts, negs, True, max_sequence_length=L, device=dev, dtype=BF)
    assert pe.shape == (2, L, cfg["d_model"]) and ne.shape == pe.shape and not torch.equal(pe, ne)
    b = pipe(prompt_embeds=pe, negative_prompt_embeds=ne, generator=torch.Generator().manual_seed(1), **kw).frames
    assert torch.isfinite(a.float()).all() and torch.equal(a, b)
    ids = StubTokenizer(cfg["vocab_size"])(prompts, max_length=L)["input_ids"]
    got = te.compute_prompt_embeddings(None, enc, None, L, dev, BF, text_input_ids=ids)
    assert torch.equal(got, enc(ids.to(dev))[0]) and torch.equal(got, pe)
