"""LoRA adapters on the GPU: the skinny transposed GEMM (orv_gemm_tn_skinny_bf16) and the adapter forward through the HIP path."""
import pytest
import torch

import lora_ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BF16 = torch.bfloat16


def _bar(got, ref):
    """The per-op bar of DESIGN.md section 1: |err| <= 1.6e-2 |ref| + 1e-2 max|ref| at every element."""
    err = (got.double().cpu() - ref).abs()
    lim = 1.6e-2 * ref.abs() + 1e-2 * ref.abs().max()
    worst = (err / lim).max().item()
    print(f"worst |err| / bar = {worst:.3f}")
    assert worst <= 1.0, f"|err| reaches {worst:.3f} x the per-op bar"


def _operands(M, P, Q, seed):
    """U [M, P] and V [M, Q] as column slices (offsets 16 / 8) of wider buffers; C [P, Q] inside a sentinel-filled wider buffer."""
    g = torch.Generator().manual_seed(seed)
    ubuf = torch.randn(M, P + 40, generator=g).to(BF16)
    vbuf = torch.randn(M, Q + 24, generator=g).to(BF16)
    cbuf = torch.full((P, Q + 8), 7.0).to(BF16)
    return ubuf, vbuf, cbuf


@pytest.mark.parametrize("M", [1, 63, 666, 4097])
@pytest.mark.parametrize("P,Q", [(16, 128), (64, 192), (192, 64), (128, 1920)])
def test_skinny_kernel_parity(M, P, Q):
    """alpha * U^T V against float64, operands as column slices, all four shapes x the four contraction lengths (one row, fewer rows
    than a 32-row MFMA k-step, a tail chunk, several 64-row stages per workgroup)."""
    from orv_amd import ops
    ubuf, vbuf, cbuf = _operands(M, P, Q, 1000 * M + P)
    alpha = 0.37
    ref = alpha * (ubuf[:, 16:16 + P].double().T @ vbuf[:, 8:8 + Q].double())
    u, v, c = ubuf.to(DEV), vbuf.to(DEV), cbuf.to(DEV)
    ops.gemm_tn_skinny(u[:, 16:], v[:, 8:], c, M, P, Q, alpha=alpha, ldu=P + 40, ldv=Q + 24, ldc=Q + 8)
    torch.cuda.synchronize()
    _bar(c[:, :Q], ref)
    assert torch.equal(c[:, Q:].cpu(), cbuf[:, Q:]), "columns of C beyond Q were written"


@pytest.mark.parametrize("P,Q", [(64, 192), (192, 64)])
def test_skinny_kernel_accumulate_and_determinism(P, Q):
    from orv_amd import ops
    M = 666
    ubuf, vbuf, _ = _operands(M, P, Q, 5)
    g = torch.Generator().manual_seed(6)
    c0 = (30.0 * torch.randn(P, Q + 8, generator=g)).to(BF16)
    alpha = -1.25
    ref = c0[:, :Q].double() + alpha * (ubuf[:, 16:16 + P].double().T @ vbuf[:, 8:8 + Q].double())
    u, v = ubuf.to(DEV), vbuf.to(DEV)
    outs = []
    for _ in range(2):
        c = c0.to(DEV)
        ops.gemm_tn_skinny(u[:, 16:], v[:, 8:], c, M, P, Q, alpha=alpha, accumulate=True, ldu=P + 40, ldv=Q + 24, ldc=Q + 8)
        outs.append(c)
    torch.cuda.synchronize()
    _bar(outs[0][:, :Q], ref)
    assert torch.equal(outs[0], outs[1]), "two runs differ"
    assert torch.equal(outs[0][:, Q:].cpu(), c0[:, Q:]), "columns of C beyond Q were written"


# ---- the model with an adapter -------------------------------------------------------------------------------------------------------
from conftest import load_golden  # noqa: E402
from oracle import dit  # noqa: E402  (checker only)
from test_gpu_training import grad_bound  # noqa: E402

CONFIGS = ["fwd_actions", "fwd_rope"]        # fused-qk projection without an adapter / RoPE (projection + orv_qkv_prep)
_cache = {}


def _gold(name):
    if name not in _cache:
        cfg, extra, ins, w, outs = load_golden(name)
        _cache[name] = dict(cfg=cfg, extra=extra, ins=ins, w=w, base=lora_ref.oracle_forward(dit, cfg, extra, ins, w), merged={})
    return _cache[name]


def _adapter(g, r):
    return lora_ref.random_adapter(g["cfg"], r, lora_ref.sigma_for(r), seed=100 + r)


def _oracle_merged(g, r, scale):
    key = (r, scale)
    if key not in g["merged"]:
        sd = lora_ref.merged_weights(g["w"], _adapter(g, r), lora_ref.coefficient(r, 2 * r, scale))
        g["merged"][key] = lora_ref.oracle_forward(dit, g["cfg"], g["extra"], g["ins"], sd)
    return g["merged"][key]


def _model(g, r=None, name="default"):
    from orv_amd.cogvideox_control import CogVideoXTransformer3DModelTraj
    m = lora_ref.build_model(CogVideoXTransformer3DModelTraj, g["cfg"], g["extra"], g["ins"], g["w"], DEV)
    if r is not None:
        lora_ref.load_adapter(m, _adapter(g, r), r, 2 * r, name=name)
    return m


def _run(m, g, **kw):
    args, kwargs = lora_ref.model_inputs(g["extra"], g["ins"], DEV)
    with torch.no_grad():
        out = m(*args, **kwargs, **kw)[0]
    torch.cuda.synchronize()
    return out


def _slice_rel_l2(got, ref):
    """Largest rel-L2 over single frames and single channels of a [B, T, C, H, W] latent (the second forward bar of the project)."""
    got, ref = got.float().cpu(), ref.float().cpu()
    d = got - ref
    per_frame = d.flatten(2).norm(dim=2) / ref.flatten(2).norm(dim=2).clamp_min(1e-12)
    per_chan = d.transpose(1, 2).flatten(2).norm(dim=2) / ref.transpose(1, 2).flatten(2).norm(dim=2).clamp_min(1e-12)
    return max(per_frame.max().item(), per_chan.max().item())


@pytest.mark.parametrize("scale", [1.0, 0.5])
@pytest.mark.parametrize("r", [8, 64])
@pytest.mark.parametrize("name", CONFIGS)
def test_forward_with_active_adapter_matches_oracle_on_merged_weights(name, r, scale):
    """Active adapter (lora_alpha = 2 r, optionally attention_kwargs scale 0.5) against the fp32 oracle run on W + c B A: rel-L2 <= 2e-2
    and worst frame / channel <= 4e-2.  A, B ~ N(0, sigma), sigma = 0.2 (8 / r)^(1/4) (lora_ref.sigma_for).  Precondition on the oracle
    alone: merged and base outputs differ by rel-L2 >= 1e-1 (five times the bar), so a forward that ignores the adapter or the scale
    fails.  Measured separations from the base (full / half strength; full vs half in brackets): fwd_actions r = 8 0.703 / 0.231 (0.503),
    r = 64 0.613 / 0.204 (0.446); fwd_rope r = 8 0.485 / 0.154 (0.347), r = 64 0.421 / 0.118 (0.325)."""
    g = _gold(name)
    ref = _oracle_merged(g, r, scale)
    sep = lora_ref.rel_l2(ref, g["base"])
    other = lora_ref.rel_l2(ref, _oracle_merged(g, r, 1.5 - scale))
    print(f"[lora-sep] {name} r={r} scale={scale}: merged vs base {sep:.3f}, vs the other strength {other:.3f}")
    assert sep >= 1e-1 and other >= 1e-1
    m = _model(g, r)
    out = _run(m, g, **({} if scale == 1.0 else {"attention_kwargs": {"scale": scale}}))
    err, worst = lora_ref.rel_l2(out.float().cpu(), ref), _slice_rel_l2(out, ref)
    print(f"[lora-fwd] {name} r={r} scale={scale}: rel-L2 {err:.2e} worst frame / channel {worst:.2e}")
    assert err <= 2e-2 and worst <= 4e-2


@pytest.mark.parametrize("name", CONFIGS)
def test_off_means_off(name):
    g = _gold(name)
    base = _run(_model(g), g)
    m = _model(g, 8)
    assert not torch.equal(_run(m, g), base)
    m.disable_adapters()
    assert torch.equal(_run(m, g), base), "disabled adapter"
    assert torch.equal(_run(m, g, attention_kwargs={"scale": 0.5}), base), "scale without an active adapter"
    m.enable_adapters()
    m.fuse_lora()
    fused_sd = {k: v.detach().float().cpu() for k, v in m.state_dict().items()}
    fused = _run(m, g)
    fresh = _model(dict(g, w=fused_sd))
    assert torch.equal(fused, _run(fresh, g)), "fused adapter vs a fresh model on the fused weights"
    m.unfuse_lora()
    assert not torch.equal(_run(m, g), base), "an unfused adapter is active again"
    m.disable_adapters()
    assert torch.equal(_run(m, g), base), "unfused, then disabled adapter"
    m.delete_adapter("default")
    assert torch.equal(_run(m, g), base), "unfused + deleted adapter"
    m = _model(g, 8)
    m.delete_adapter("default")                  # an active adapter that was never fused or disabled
    assert m.active_adapter is None and torch.equal(_run(m, g), base), "deleted active adapter"


def _grads(m, g, wout):
    args, kwargs = lora_ref.model_inputs(g["extra"], g["ins"], DEV)
    out = m(*args, **kwargs)[0]
    assert out.requires_grad
    (out.float() * wout.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name,r", [(CONFIGS[0], 16), (CONFIGS[1], 16), (CONFIGS[0], 8)])
def test_adapter_gradients_match_oracle_autograd(name, r):
    """Every adapter tensor's gradient (r = 16, random nonzero B) against torch autograd through the oracle on W + c B A with A, B as
    leaves; bound: test_gpu_training.grad_bound (3e-2 for the weight family), no tensor skipped.  Base parameters get no gradient, and
    gradient checkpointing gives bit-identical adapter gradients.  (r = 8: a rank below the kernel's multiple of 16 - the gradient is
    computed into a padded temporary and sliced.)"""
    g = _gold(name)
    c = lora_ref.coefficient(r, 2 * r)
    leaves = {k: (A.clone().requires_grad_(True), B.clone().requires_grad_(True)) for k, (A, B) in _adapter(g, r).items()}
    torch.manual_seed(0)
    wout = torch.randn(g["base"].shape)
    ref_out = lora_ref.oracle_forward(dit, g["cfg"], g["extra"], g["ins"], lora_ref.merged_weights(g["w"], leaves, c))
    (ref_out * wout).sum().backward()
    m = _model(g, r).train()
    out = _grads(m, g, wout)
    assert lora_ref.rel_l2(out.detach().float().cpu(), ref_out.detach()) <= 2e-2
    ad = m._lora_adapters["default"]
    errs = []
    for k, (A, B) in ad.params.items():
        for p, leaf, tag in ((A, leaves[k][0], "lora_A"), (B, leaves[k][1], "lora_B")):
            assert p.grad is not None and p.grad.shape == p.shape, (k, tag)
            errs.append((lora_ref.rel_l2(p.grad.float().cpu(), leaf.grad), f"{k}.{tag}"))
    errs.sort()
    print(f"[lora-grad-err] {name} r={r}: n={len(errs)} median={errs[len(errs) // 2][0]:.2e} p90={errs[int(len(errs) * 0.9)][0]:.2e} "
          f"max={errs[-1][0]:.2e} ({errs[-1][1]})")
    own = {id(p) for ab in ad.params.values() for p in ab}
    assert all(p.grad is None for p in m.parameters() if id(p) not in own), "a frozen base parameter received a gradient"
    bad = [(k, round(e, 4)) for e, k in errs if e > grad_bound(k)]
    assert all(grad_bound(k) == 3e-2 for _, k in errs), "adapter tensors belong to the weight family"
    assert len(errs) == 2 * 4 * g["cfg"]["num_layers"] and not bad, bad
    resident = {k: (A.grad.clone(), B.grad.clone()) for k, (A, B) in ad.params.items()}
    m.zero_grad(set_to_none=True)
    m.enable_gradient_checkpointing()
    _grads(m, g, wout)
    for k, (A, B) in ad.params.items():
        assert torch.equal(A.grad, resident[k][0]) and torch.equal(B.grad, resident[k][1]), k


@pytest.mark.parametrize("precision", ["bf16", "split_fp32"])
def test_adapter_training_steps(precision):
    """FusedAdamW over the trainable parameters of a fresh adapter (B = 0): its flat buffer holds the adapter segments only, three steps
    leave every base weight untouched and lower the loss on the fixed batch."""
    from orv_amd.optim import FusedAdamW
    g = _gold("fwd_actions")
    m = _model(g).train()
    m.add_adapter(r=16, lora_alpha=32)
    base0 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    params = [p for p in m.parameters() if p.requires_grad]
    assert len(params) == 2 * 4 * g["cfg"]["num_layers"]
    opt = FusedAdamW(params, lr=1e-2, betas=(0.9, 0.95), weight_decay=0.0, max_grad_norm=1.0, param_precision=precision)
    args, kwargs = lora_ref.model_inputs(g["extra"], g["ins"], DEV)
    torch.manual_seed(3)
    target = torch.randn(g["base"].shape).to(DEV)
    losses = []
    for _ in range(4):
        out = m(*args, **kwargs)[0]
        loss = (out.float() - target).square().mean()
        losses.append(loss.item())
        if len(losses) == 4:
            break
        loss.backward()
        opt.step()
        opt.zero_grad()
    seg = 0
    for p in params:
        assert p.data_ptr() >= opt._flat["p"].data_ptr() and p.data_ptr() < opt._flat["p"].data_ptr() + opt._flat["p"].numel() * 2
        seg += p.numel()
    assert seg <= opt._flat["p"].numel() < seg + 2048 * len(params), "the flat parameter buffer holds more than the adapter segments"
    now = m.state_dict()
    assert all(torch.equal(now[k], base0[k]) for k in base0), "a base weight moved"
    print(f"[lora-train] {precision}: losses {losses}")
    assert losses[-1] < losses[0], losses


def test_graph_replay_follows_adapter_state():
    from orv_amd.cogvideox_control import CogVideoXImageToVideoPipelineTraj as Pipe
    g = _gold("fwd_actions")
    m = _model(g, 8)
    lora_ref.load_adapter(m, lora_ref.random_adapter(g["cfg"], 8, 0.2, seed=77), 8, 16, name="other")
    m.set_adapter("default")
    pipe = Pipe(transformer=m).enable_hip_graph(True)
    args, _ = lora_ref.model_inputs(g["extra"], g["ins"], DEV)
    kw = dict(hidden_states=args[0], encoder_hidden_states=args[1], controls_or_guidances=args[2], timestep=args[3], return_dict=False)

    def replayed(**extra):
        outs = [pipe.transformer_forward(**kw, **extra)[0].clone() for _ in range(3)]      # eager warm-up, capture, replay
        torch.cuda.synchronize()
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
        return outs[2]
    first = replayed()
    assert torch.equal(first, _run(m, g)), "replay vs eager"
    with torch.no_grad():
        B = m._lora_adapters["default"].params["transformer_blocks.1.attn1.to_v"][1]
        B.copy_(B * 1.5)
    after = replayed()
    assert not torch.equal(after, first) and torch.equal(after, _run(m, g)), "in-place edit of one B"
    half = replayed(attention_kwargs={"scale": 0.5})
    assert not torch.equal(half, after) and torch.equal(half, _run(m, g, attention_kwargs={"scale": 0.5})), "new scale"
    m.set_adapter("other")
    other = replayed()
    assert not torch.equal(other, after) and torch.equal(other, _run(m, g)), "set_adapter"


def test_mxfp8_refuses_an_unfused_adapter_and_runs_a_fused_one():
    g = _gold("fwd_actions")
    m = _model(g, 8)
    with pytest.raises(RuntimeError, match="fuse"):
        m.enable_mxfp8()
    m.fuse_lora()
    m.enable_mxfp8()
    out = _run(m, g)
    ref = _oracle_merged(g, 8, 1.0)
    assert torch.isfinite(out.float()).all() and lora_ref.rel_l2(out.float().cpu(), ref) < 0.2
    with pytest.raises(RuntimeError):
        m.unfuse_lora(), _run(m, g)
