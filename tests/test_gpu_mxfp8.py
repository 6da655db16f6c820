"""MXFP8 inference mode on the MI355X: the quantiser and the LayerNorm producer bit for bit against the CPU restatement
(tests/mxfp8_ref.py), the block-scaled GEMM against dequantised fp32 products, and the model path against an emulated-MXFP8 oracle.
Accuracy lines are printed with the prefix ``[mxfp8]`` (recorded in profiles/mxfp8_accuracy.txt)."""
import math
import os

import pytest
import torch

import mxfp8_ref

pytestmark = pytest.mark.gpu

from oracle import dit  # noqa: E402  (checker only)

BF = torch.bfloat16
DEV = torch.device("cuda:0")


def rel_l2(got, ref):
    got, ref = got.float().cpu(), ref.float().cpu()
    return ((got - ref).norm() / ref.norm()).item()


def _edge_rows(K):
    """Rows of edge-case blocks (all-zero, amax exactly 448 * 2^e and just above, e4m3 subnormals after scaling, +-max bf16, -0)."""
    mx = torch.tensor(0x7F7F, dtype=torch.int16).view(BF).item()
    rows = []
    for vals in ([0.0], [-0.0, 0.0], [448.0 * 8, 1.0, -0.001], [450.0 * 8, 3 * 2 ** -10, -(2 ** -10)], [448.0, 0.001, 2 ** -10, -0.0],
                 [mx, -mx, 1.0], [2.0 ** -130, -(2.0 ** -133)], [1e-20, 3e-21]):
        blk = torch.zeros(32)
        blk[:len(vals)] = torch.tensor(vals)
        rows.append(blk.repeat(K // 32))
    return torch.stack(rows)


def _data(M, K, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g) * torch.pow(2.0, torch.randint(-24, 24, (M, 1), generator=g).float())
    e = _edge_rows(K)
    x[:e.shape[0]] = e
    x[-1, 32:64] = 0.0                                      # an all-zero block inside a random row
    return x.to(BF)


@pytest.mark.parametrize("M,K", [(333, 1920), (333, 3072), (333, 7680), (333, 12288), (3226, 1920), (3226, 7680), (12904, 1920),
                                 (12904, 3072)])
def test_quantize_bit_exact(M, K):
    x = _data(M, K, M + K)
    q, s = mxfp8_ref.quantize(x)
    from orv_amd import ops
    xd = x.to(DEV)
    gq, gs = ops.mxfp8_quantize(xd)
    torch.cuda.synchronize()
    assert torch.equal(gs.cpu(), s)
    assert torch.equal(gq.cpu(), q)
    # strided source rows (ldx > K)
    big = torch.zeros(M, K + 64, dtype=BF, device=DEV)
    big[:, :K] = xd
    gq2, gs2 = ops.mxfp8_quantize(big, M, K, ldx=K + 64)
    assert torch.equal(gq2.cpu(), q) and torch.equal(gs2.cpu(), s)


@pytest.mark.parametrize("D,B,S,Nt,P", [(1920, 2, 3226, 226, 600), (3072, 1, 1762, 226, 192), (128, 2, 80, 8, 24)])
def test_layernorm_modulate_mxfp8_is_bf16_then_quantize(D, B, S, Nt, P):
    """The fused producer writes exactly the bytes of LayerNorm-modulate (bf16) followed by the quantiser, on the model's token-group
    modulation layout (text group + one group per frame, tables [B, G, 3D] fp32)."""
    from orv_amd import ops
    g = torch.Generator().manual_seed(D + S)
    G = 1 + (S - Nt) // P
    x = (torch.randn(B * S, D, generator=g) * 3).to(BF).to(DEV)
    x[5] = 0.0                                                              # a constant row: LayerNorm output = beta-only
    gamma = (1 + 0.1 * torch.randn(D, generator=g)).to(BF).to(DEV)
    beta = (0.1 * torch.randn(D, generator=g)).to(BF).to(DEV)
    tab = (0.5 * torch.randn(B, G, 3 * D, generator=g)).to(DEV)
    grp = ops.groups(S, Nt, P)
    mb, mg = G * 3 * D, 3 * D
    y = torch.empty(B * S, D, dtype=BF, device=DEV)
    ops.layernorm_modulate(x, y, gamma, beta, tab[..., D:2 * D], tab[..., :D], mb, mg, grp, B, D, 1e-5)
    q0, s0 = ops.mxfp8_quantize(y)
    q1 = torch.empty(B * S, D, dtype=torch.uint8, device=DEV)
    s1 = torch.empty(B * S, D // 32, dtype=torch.uint8, device=DEV)
    ops.layernorm_modulate_mxfp8(x, q1, s1, gamma, beta, tab[..., D:2 * D], tab[..., :D], mb, mg, grp, B, D, 1e-5)
    torch.cuda.synchronize()
    assert torch.equal(s1, s0) and torch.equal(q1, q0)
    q2, s2 = mxfp8_ref.quantize(y.cpu())
    assert torch.equal(q1.cpu(), q2) and torch.equal(s1.cpu(), s2)


def _gemm(qa, sa, qw, sw, M, N, K, bias=None, epilogue=0, **kw):
    from orv_amd import ops
    C = kw.pop("C", None)
    if C is None:
        C = torch.empty(M, N, dtype=BF, device=DEV)
    ops.gemm_mxfp8(qa.to(DEV), sa.to(DEV), qw.to(DEV), sw.to(DEV), bias, C, M, N, K, epilogue=epilogue, **kw)
    torch.cuda.synchronize()
    return C


def test_lane_map_exact_integers():
    """Small integers with unit scales and an asymmetric W: every product and sum is exact, so must be C."""
    M, N, K = 333, 256, 256
    i = torch.arange(M)[:, None]
    k = torch.arange(K)[None, :]
    n = torch.arange(N)[:, None]
    A = ((i * 3 + k * 7 + (i * k) % 5) % 3 - 1).float()                  # {-1, 0, 1}
    W = ((n * 5 + k * k + 2 * (n > k).long()) % 3 - 1).float()            # asymmetric in (n, k)
    qa = A.to(mxfp8_ref.E4M3).view(torch.uint8)
    qw = W.to(mxfp8_ref.E4M3).view(torch.uint8)
    sa = torch.full((M, K // 32), 127, dtype=torch.uint8)
    sw = torch.full((N, K // 32), 127, dtype=torch.uint8)
    C = _gemm(qa, sa, qw, sw, M, N, K)
    assert torch.equal(C.float().cpu(), A @ W.t())


def _bound(ref, absprod, K):
    # bf16 output rounding + the worst case of a K-term fp32 sum (K 2^-23 of the sum of |products|): the scales span 2^120 here, so the
    # products of one output meet at wildly different magnitudes; a misrouted scale is off by factors up to 2^60
    return ref.abs() * 2.0 ** -8 + K * 2.0 ** -23 * absprod


def test_scale_routing():
    """A different e8m0 scale on every (row, 32-block) of A and W, 2^-30 .. 2^30: against the fp32 product of the dequantised operands."""
    M, N, K = 333, 256, 1024
    g = torch.Generator().manual_seed(5)
    qa = torch.randint(0, 256, (M, K), generator=g, dtype=torch.uint8)
    qw = torch.randint(0, 256, (N, K), generator=g, dtype=torch.uint8)
    qa[(qa & 0x7F) == 0x7F] = 0x38                                         # no NaN encodings
    qw[(qw & 0x7F) == 0x7F] = 0x38
    sa = torch.randint(127 - 30, 127 + 31, (M, K // 32), generator=g, dtype=torch.uint8)
    sw = torch.randint(127 - 30, 127 + 31, (N, K // 32), generator=g, dtype=torch.uint8)
    Ad, Wd = mxfp8_ref.dequantize(qa, sa), mxfp8_ref.dequantize(qw, sw)
    ref = Ad @ Wd.t()
    absprod = Ad.abs() @ Wd.abs().t()
    C = _gemm(qa, sa, qw, sw, M, N, K).double().cpu()
    err = (C - ref).abs()
    print(f"[mxfp8] scale routing: max |C - ref| / (|A| |W|^T) = {float((err / absprod).max()):.3e}, "
          f"median = {float((err / absprod).median()):.3e}")
    assert (err <= _bound(ref, absprod, K)).all()
    # a permuted scale (other row, other block) must be seen
    sw2 = sw.clone()
    sw2[:, 0], sw2[:, 1] = sw[:, 1], sw[:, 0]
    C2 = _gemm(qa, sa, qw, sw2, M, N, K).double().cpu()
    assert not ((C2 - ref).abs() <= _bound(ref, absprod, K)).all()


def _gelu(x):
    return 0.5 * x * (1 + torch.tanh(math.sqrt(2 / math.pi) * (x + 0.044715 * x ** 3)))


@pytest.mark.parametrize("M,N,K", [(3226, 5760, 1920), (3226, 1920, 1920), (12904, 7680, 1920), (12904, 1920, 7680), (1762, 3072, 3072),
                                   (1762, 12288, 3072), (333, 1920, 7680)])
@pytest.mark.parametrize("epilogue", [0, 1, 2])
def test_gemm_vs_dequantised_matmul(M, N, K, epilogue):
    from orv_amd import ops
    g = torch.Generator(device=DEV).manual_seed(M + N + K + epilogue)
    A = torch.randn(M, K, device=DEV, generator=g).to(BF)
    W = (0.02 * torch.randn(N, K, device=DEV, generator=g)).to(BF)
    bias = (0.1 * torch.randn(N, device=DEV, generator=g)).to(BF)
    qa, sa = ops.mxfp8_quantize(A)
    qw, sw = ops.mxfp8_quantize(W)
    Ad = mxfp8_ref.fake_quant(A)
    Wd = mxfp8_ref.fake_quant(W)
    acc = Ad @ Wd.t() + bias.float()
    absprod = Ad.abs() @ Wd.abs().t()
    kw = {}
    if epilogue == 0:
        ref, slack = acc, 1e-5 * absprod
    elif epilogue == 1:
        ref, slack = _gelu(acc), 1.2e-5 * absprod + 1e-6
    else:
        S = M // 2 if M % 2 == 0 else M
        B = M // S
        Nt, P = 26, 100
        G = 1 + -(-(S - Nt) // P)
        R = torch.randn(M, N, device=DEV, generator=g).to(BF)
        gate = torch.randn(B, G, N, device=DEV, generator=g)
        s_idx = torch.arange(M, device=DEV) % S
        grp_idx = torch.where(s_idx < Nt, 0, 1 + (s_idx - Nt) // P)
        gr = gate[torch.arange(M, device=DEV) // S, grp_idx]
        ref = R.float() + gr * acc
        slack = gr.abs() * 1e-5 * absprod
        kw = dict(R=R, ldr=N, gate=gate, gate_b=G * N, gate_g=N, grp=ops.groups(S, Nt, P))
    C = torch.empty(M, N, dtype=BF, device=DEV)
    ops.gemm_mxfp8(qa, sa, qw, sw, bias, C, M, N, K, epilogue=epilogue, **kw)
    torch.cuda.synchronize()
    err = (C.float() - ref).abs()
    bound = ref.abs() * 2.0 ** -8 + slack + 1e-6
    assert (err <= bound).all(), float((err - bound).max())


# ---- the model path ----------------------------------------------------------------------------------------------------------------
_MX_LINEARS = (".attn1.to_q", ".attn1.to_k", ".attn1.to_v", ".attn1.to_out.0", ".ff.net.0.proj", ".ff.net.2")


def _emulated_lin(orig):
    """oracle.dit._lin with the six block linears on MXFP8: bf16(x) and the weight quantised with the CPU restatement's rule."""
    cache = {}

    def lin(sd, name, x):
        if name.startswith("transformer_blocks.") and name.endswith(_MX_LINEARS):
            w = sd[name + ".weight"]
            key = (name, w.data_ptr())
            if key not in cache:
                cache[key] = mxfp8_ref.fake_quant(w)
            return torch.nn.functional.linear(mxfp8_ref.fake_quant(x), cache[key], sd.get(name + ".bias"))
        return orig(sd, name, x)
    return lin


def test_full_width_single_layer_vs_emulated_oracle(monkeypatch):
    """CogVideoX-2B widths, one block, B = 1 (as test_gpu_model.py::test_full_width_single_layer_vs_oracle) on the MXFP8 path against
    the oracle with the same six linears on MXFP8: rel-L2 <= 2e-2; the distance to the plain fp32 oracle is printed."""
    from orv_amd.cogvideox_control import CogVideoXTransformer3DModelTraj
    torch.manual_seed(42)
    cfg = dict(num_layers=1, in_channels=32, sample_height=40, sample_width=60, sample_frames=17, modulate_encoder_hidden_states=True)
    m = CogVideoXTransformer3DModelTraj(**cfg)
    for p in m.parameters():
        if p.ndim >= 2:
            p.data.normal_(0, 0.02)
        p.data.copy_(p.data.to(BF).float())
    x = torch.randn(1, 5, 32, 40, 60).to(BF).float()
    e = (torch.randn(1, 226, 4096) * 0.2).to(BF).float()
    a = torch.randn(1, 16, 7).to(BF).float()
    ts = torch.tensor([500])
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    args = (dict(m.config), x, e, ts)
    with torch.no_grad():
        ref = dit.dit_forward(sd, *args, actions=a, is_mask=torch.zeros(1, dtype=torch.bool))[0]
        monkeypatch.setattr(dit, "_lin", _emulated_lin(dit._lin))
        ref_mx = dit.dit_forward(sd, *args, actions=a, is_mask=torch.zeros(1, dtype=torch.bool))[0]
    m = m.to(DEV, BF).eval().enable_mxfp8()
    m.action_embed.forced_mask = torch.zeros(1, dtype=torch.bool)
    with torch.no_grad():
        out = m(x.to(DEV, BF), e.to(DEV, BF), {"actions": a.to(DEV)}, ts.to(DEV), return_dict=False)[0]
    err_mx, err_fp = rel_l2(out, ref_mx), rel_l2(out, ref)
    print(f"[mxfp8] 2B single block B=1: rel-L2 vs emulated-MXFP8 oracle = {err_mx:.4e}, vs fp32 oracle = {err_fp:.4e}, "
          f"emulated vs fp32 oracle = {rel_l2(ref_mx, ref):.4e}")
    assert err_mx <= 2e-2


def test_full_depth_2b_vs_emulated_oracle_and_batch_consistency(monkeypatch):
    """All 30 blocks of CogVideoX-2B (bench weights / inputs, S = 3226) on the MXFP8 path: B = 4 equals four B = 1 calls bit for bit, and
    the t = 500 clip is close to the emulated-MXFP8 oracle (distance to the fp32 oracle printed).
    Bar: 3e-2, or 1.25 x the distance between the emulated oracle and the same emulated oracle fed bf16-rounded latents perturbed by one
    bf16 step, where that is larger.  Measured (profiles/mxfp8_accuracy.txt, tools/mxfp8_drift.py): two MXFP8 computations whose inputs
    differ at bf16 resolution land 5.4e-2 apart after 30 blocks (the fp32 model under the same perturbation: 5.2e-4) - quantisation-
    boundary flips (an e4m3 step is 1/8 of the value) amplified through the blocks; no implementation that is not bit-identical to the
    emulation can meet the guessed 3e-2 there, and the HIP path sits at 1.06 x that distance."""
    import bench
    cfg = dict(bench.CFG_2B)
    model = bench.build_model(cfg, DEV).enable_mxfp8()
    lat, img, prompt, actions = bench.synthetic_inputs(4, DEV, BF)
    x = torch.cat([lat, img], dim=2)
    ts = torch.tensor([500, 999, 19, 259], device=DEV)
    with torch.no_grad():
        model.action_embed.forced_mask = torch.zeros(4, dtype=torch.bool)
        out4 = model(x, prompt, {"actions": actions}, ts, return_dict=False)[0].cpu()
        model.action_embed.forced_mask = torch.zeros(1, dtype=torch.bool)
        singles = [model(x[b:b + 1], prompt[b:b + 1], {"actions": actions[b:b + 1]}, ts[b:b + 1], return_dict=False)[0].cpu()
                   for b in range(4)]
    for b in range(4):
        assert torch.equal(out4[b:b + 1], singles[b]), b
    sd = {k: v.detach().float().cpu() for k, v in model.state_dict().items()}
    torch.set_num_threads(max(1, min(16, (os.cpu_count() or 2) // 2)))
    b = 0
    oargs = (sd, dict(model.config), x[b:b + 1].float().cpu(), prompt[b:b + 1].float().cpu(), ts[b:b + 1].cpu())
    okw = dict(actions=actions[b:b + 1].float().cpu(), is_mask=torch.zeros(1, dtype=torch.bool))
    g = torch.Generator().manual_seed(1)
    xp = (oargs[2] * (1 + 2.0 ** -9 * torch.randn(oargs[2].shape, generator=g))).to(BF).float()
    with torch.no_grad():
        ref = dit.dit_forward(*oargs, **okw)[0]
        monkeypatch.setattr(dit, "_lin", _emulated_lin(dit._lin))
        ref_mx = dit.dit_forward(*oargs, **okw)[0]
        ref_mxp = dit.dit_forward(oargs[0], oargs[1], xp, *oargs[3:], **okw)[0]
    err_mx, err_fp, flips = rel_l2(singles[b], ref_mx), rel_l2(singles[b], ref), rel_l2(ref_mxp, ref_mx)
    print(f"[mxfp8] 2B full depth (30 blocks) t=500: rel-L2 vs emulated-MXFP8 oracle = {err_mx:.4e}, vs fp32 oracle = {err_fp:.4e}, "
          f"emulated vs fp32 oracle = {rel_l2(ref_mx, ref):.4e}, emulated vs emulated with bf16-step input perturbation = {flips:.4e}")
    assert err_mx <= max(3e-2, 1.25 * flips)


def _tiny(name="fwd_actions"):
    from conftest import load_golden
    from orv_amd.cogvideox_control import CogVideoXTransformer3DModelTraj
    cfg, extra, ins, w, outs = load_golden(name)
    m = CogVideoXTransformer3DModelTraj(**cfg)
    m.load_state_dict(w, strict=True)
    m = m.to(DEV, BF).eval().requires_grad_(False)
    m.action_embed.forced_mask = torch.tensor(extra["mask"])
    args = (ins["hidden_states"].to(DEV, BF), ins["encoder_hidden_states"].to(DEV, BF), {"actions": ins["actions"].to(DEV)},
            ins["timestep"].to(DEV))
    return m, args, ins


def test_stale_weights_are_requantised():
    m, args, _ = _tiny()
    m.enable_mxfp8()
    out0 = m(*args, return_dict=False)[0].clone()
    with torch.no_grad():
        m.transformer_blocks[1].ff.net[0].proj.weight.mul_(1.5)               # in place: _version moves, storage stays
    out1 = m(*args, return_dict=False)[0].clone()
    fresh, _, _ = _tiny()
    fresh.load_state_dict(m.state_dict())
    fresh.enable_mxfp8()
    out2 = fresh(*args, return_dict=False)[0]
    assert torch.equal(out1, out2)
    assert not torch.equal(out0, out1)
    # a replaced Parameter
    blk = m.transformer_blocks[0].attn1.to_out[0]
    blk.weight = torch.nn.Parameter(blk.weight.detach() * 0.5, requires_grad=False)
    out3 = m(*args, return_dict=False)[0].clone()
    with torch.no_grad():
        fresh.transformer_blocks[0].attn1.to_out[0].weight.mul_(0.5)
    assert torch.equal(out3, fresh(*args, return_dict=False)[0]) and not torch.equal(out3, out1)


def test_rope_path_and_disable_is_bit_identical():
    """RoPE (qk LayerNorm + RoPE through orv_qkv_prep) runs, and enable_mxfp8(False) returns to the bf16 path bit for bit."""
    m, args, ins = _tiny("fwd_rope")
    rope = (ins["rope_cos"].to(DEV), ins["rope_sin"].to(DEV))
    never, _, _ = _tiny("fwd_rope")
    ref = never(*args, image_rotary_emb=rope, return_dict=False)[0]
    mx = m.enable_mxfp8()(*args, image_rotary_emb=rope, return_dict=False)[0].clone()
    assert not torch.equal(mx, ref) and rel_l2(mx, ref) <= 5e-2
    back = m.enable_mxfp8(False)(*args, image_rotary_emb=rope, return_dict=False)[0]
    assert torch.equal(back, ref)


def test_hip_graph_with_mxfp8():
    """Pipeline replayed from the HIP graph == eager with MXFP8 on; enabling after a bf16 capture changes the output; disabling again
    replays the bf16 result bit for bit."""
    from conftest import load_golden
    from orv_amd import schedulers
    from orv_amd.cogvideox_control import CogVideoXImageToVideoPipelineTraj, CogVideoXTransformer3DModelTraj
    cfg, extra, ins, w, outs = load_golden("pipe_ddim")
    m = CogVideoXTransformer3DModelTraj(**cfg)
    m.load_state_dict(w, strict=True)
    m = m.to(DEV, BF).eval()
    b = ins["image"].shape[0]
    m.action_embed.forced_mask = torch.zeros(b, dtype=torch.bool)
    g = torch.Generator().manual_seed(3)
    image_lat = torch.randn(b, 16, 1, 8, 12, generator=g).to(DEV, BF)
    lat0 = torch.randn(b, 3, 16, 8, 12, generator=g).to(DEV, BF)

    def run(graph):
        sched = schedulers.CogVideoXDDIMScheduler(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012,
                                                  beta_schedule="scaled_linear", prediction_type="v_prediction",
                                                  rescale_betas_zero_snr=True, snr_shift_scale=3.0, timestep_spacing="trailing")
        pipe = CogVideoXImageToVideoPipelineTraj(transformer=m, scheduler=sched).enable_hip_graph(graph)
        out = pipe(image=image_lat, height=64, width=96, num_frames=9, num_inference_steps=4, guidance_scale=1.0,
                   latents=lat0.clone(), prompt_embeds=ins["prompt_embeds"].to(DEV, BF), output_type="latent",
                   controls_or_guidances={"actions": ins["actions"].to(DEV)})
        return out.frames.clone()

    bf_eager = run(False)
    bf_graph = run(True)                     # captures the bf16 graph
    assert torch.equal(bf_eager, bf_graph)
    m.enable_mxfp8()
    mx_graph = run(True)
    mx_eager = run(False)
    assert torch.equal(mx_graph, mx_eager)
    assert not torch.equal(mx_graph, bf_graph)
    m.enable_mxfp8(False)
    assert torch.equal(run(True), bf_graph)
