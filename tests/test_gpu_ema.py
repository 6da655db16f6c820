"""GPU: the weight-average kernels (``orv_ema_update``, ``orv_ema_swap_in``) and ``orv_amd.FusedEMA`` against their numpy restatement
(tests/ema_ref.py), bit for bit: the update on a flat buffer of four workgroups with padding, the swap for evaluation, three ``sft_step``
calls on the small golden-config model (all parameters, and a rank-16 LoRA adapter as the only trainable set), checkpoints."""
import numpy as np
import pytest
import torch

import adamw_ref
import ema_ref as R
import lora_ref

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
DEV = torch.device("cuda:0")
SIZES = [1, 2047, 2049]          # segments of 2048, 2048, 4096 elements: four workgroups, 4095 elements of padding


def _u32(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy().view(np.uint32).reshape(-1)


def _wide(rng, n):
    """n fp32 values of random sign with magnitudes spread over 2^-60 .. 2^60."""
    return (np.ldexp(1.0 + rng.random(n), rng.integers(-60, 61, n)) * rng.choice([-1.0, 1.0], n)).astype(np.float32)


def _optimizer(precision, seed=0):
    """FusedAdamW over three parameters of SIZES elements and a FusedEMA over it, then - written through the flat buffers, which moves no
    parameter version - masters and shadows of wide magnitude with signed zeros and denormals in front of and behind the workgroup
    boundary of the last parameter.  -> (optimizer, ema, boolean map of the elements that belong to a parameter)."""
    from orv_amd import FusedEMA
    from orv_amd.optim import FusedAdamW
    rng = np.random.default_rng(seed)
    params = [torch.nn.Parameter(torch.zeros(n, dtype=BF, device=DEV)) for n in SIZES]
    opt = FusedAdamW(params, param_precision=precision)
    ema = FusedEMA(opt)
    f = opt._flat
    total = f["p"].numel()
    assert total == 8192 and f["offs"] == [0, 2048, 4096]
    inside = np.zeros(total, dtype=bool)
    for n, o in zip(SIZES, f["offs"]):
        inside[o:o + n] = True
        theta, s = _wide(rng, n), _wide(rng, n)
        if n == 2049:
            den = rng.integers(1, 1 << 23, 64).astype(np.uint32) | (rng.integers(0, 2, 64).astype(np.uint32) << np.uint32(31))
            for a in (0, 1900):
                s[a:a + 64] = den.view(np.float32)                                     # denormal shadows ...
                theta[a:a + 64:4] = 0.0                                                # ... against +0, -0, a denormal and a normal master
                theta[a + 1:a + 64:4] = -0.0
                theta[a + 2:a + 64:4] = (den[2::4] ^ np.uint32(0x80000000)).view(np.float32)
            s[2040:2049] = np.array([0.0, -0.0] * 4 + [-0.0], dtype=np.float32)        # signed zeros up to and across the workgroup boundary
            theta[2044:2049] = np.array([0.0, -0.0, -0.0, 0.0, 0.0], dtype=np.float32)  # (element 2048 is the next workgroup's only one)
        if precision == "split_fp32":
            p, lo = adamw_ref.split(torch.from_numpy(theta))                           # tie-away split: the master is theta exactly
            assert torch.equal(adamw_ref.rebuild(p, lo), torch.from_numpy(theta)) and (n == 1 or int((lo != 0).sum()) > n // 2)
            f["lo"][o:o + n] = lo.to(DEV)
        else:
            p = R.bf16_of_bits(R.bf16_rne(theta))
        f["p"][o:o + n] = p.to(DEV)
        ema.shadow[o:o + n] = torch.from_numpy(s).to(DEV)
    return opt, ema, inside


def _flat_cpu(opt):
    f = opt._flat
    return R.bits_of_bf16(f["p"]), (f["lo"].cpu().numpy() if "lo" in f else None)


@pytest.mark.parametrize("decay", [0.0, 0.5, 0.9999, 1.0])
@pytest.mark.parametrize("precision", ["bf16", "split_fp32"])
def test_update_kernel_equals_the_restatement_bit_for_bit(precision, decay):
    """Two ``FusedEMA.step()`` calls: the first runs at decay 0 (omd = 1) whatever the settings, the second at ``decay`` (cap = floor =
    ``decay``).  The whole flat shadow, padding included, must equal ema_ref.update; the padding must still be zero."""
    opt, ema, inside = _optimizer(precision)
    ema.decay = ema.min_decay = decay
    p_bits, lo = _flat_cpu(opt)
    want = ema.shadow.cpu().numpy().copy()
    assert int(((want.view(np.uint32) & 0x7F800000) == 0).sum()) >= 128 + 9 + 4095      # denormal / zero shadows (and the padding)
    for k, omd in ((1, np.float32(1.0)), (2, R.omd_of(decay))):
        ema.step()
        torch.cuda.synchronize()
        assert ema.cur_decay_value == (0.0 if k == 1 else decay)
        want = R.update(want, p_bits, lo, omd)
        got = _u32(ema.shadow)
        bad = np.flatnonzero(got != want.view(np.uint32))
        assert bad.size == 0, (k, bad[:8], got[bad[:8]], want.view(np.uint32)[bad[:8]])
        assert not got[~inside].any(), "padding of the shadow moved"
        assert np.isfinite(want).all()
    assert np.array_equal(R.bits_of_bf16(opt._flat["p"]), p_bits)                        # the update writes the shadow only
    if lo is not None:
        assert np.array_equal(opt._flat["lo"].cpu().numpy(), lo)


@pytest.mark.parametrize("precision", ["bf16", "split_fp32"])
def test_store_copy_to_restore(precision):
    from orv_amd import _state
    opt, ema, inside = _optimizer(precision, seed=1)
    f = opt._flat
    # rounding cases in the shadow: exact ties (to even: down / up), the largest finite fp32 (rounds to infinity), infinities, a NaN, -0, a denormal
    special = np.array([0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000, 0x7FC00001, 0x7F800001,
                        0x80000000, 0x00000001, 0x3F807FFF, 0x3F808001], dtype=np.uint32)
    ema.shadow[4096 + 100:4096 + 100 + special.size] = torch.from_numpy(special.view(np.float32).copy()).to(DEV)
    s = ema.shadow.cpu().numpy().copy()
    want = R.bf16_rne(s)
    assert list(want[4096 + 100:4096 + 104]) == [0x3F80, 0x3F82, 0xBF80, 0xBF82] and want[4096 + 104] == 0x7F80 and want[4096 + 109] == 0x7FC0
    p0, lo0 = _flat_cpu(opt)
    epoch = _state.weights_epoch[0]
    with ema.average_parameters():
        torch.cuda.synchronize()
        assert _state.weights_epoch[0] > epoch
        p1, lo1 = _flat_cpu(opt)
        assert np.array_equal(p1, want), np.flatnonzero(p1 != want)[:8]
        assert not p1[~inside].any()
        assert lo0 is None or np.array_equal(lo1, lo0)
        with pytest.raises(RuntimeError, match=r"FusedEMA.step: the averaged weights are swapped in"):
            ema.step()
        with pytest.raises(RuntimeError, match=r"FusedEMA.store: a stash is already held"):
            ema.store()
        epoch = _state.weights_epoch[0]
    torch.cuda.synchronize()
    assert _state.weights_epoch[0] > epoch
    p2, lo2 = _flat_cpu(opt)
    assert np.array_equal(p2, p0) and (lo0 is None or np.array_equal(lo2, lo0))
    assert np.array_equal(_u32(ema.shadow), s.view(np.uint32))
    # the three calls by hand, then copy_to outside a pair
    ema.store()
    ema.copy_to()
    torch.cuda.synchronize()
    assert np.array_equal(_flat_cpu(opt)[0], want) and (lo0 is None or np.array_equal(_flat_cpu(opt)[1], lo0))
    ema.restore()
    torch.cuda.synchronize()
    p3, lo3 = _flat_cpu(opt)
    assert np.array_equal(p3, p0) and (lo0 is None or np.array_equal(lo3, lo0))
    ema.copy_to()
    torch.cuda.synchronize()
    p4, lo4 = _flat_cpu(opt)
    assert np.array_equal(p4, want) and (lo4 is None or not lo4.any())
    assert ema._stash is None


# ---- in the model ----
from conftest import load_golden  # noqa: E402

_gold = {}


def _golden():
    if not _gold:
        cfg, extra, ins, w, outs = load_golden("fwd_actions")
        _gold.update(cfg=cfg, extra=extra, ins=ins, w=w)
    return _gold


def _fresh(g, lora):
    from orv_amd.cogvideox_control import CogVideoXTransformer3DModelTraj
    m = lora_ref.build_model(CogVideoXTransformer3DModelTraj, g["cfg"], g["extra"], g["ins"], g["w"], DEV)
    if lora:
        m.add_adapter(r=16, lora_alpha=32)
    return m


def _forward(m, g):
    args, kwargs = lora_ref.model_inputs(g["extra"], g["ins"], DEV)
    with torch.no_grad():
        out = m(*args, **kwargs)[0].clone()
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("case", ["all_split_fp32", "all_bf16", "lora_r16_split_fp32"])
def test_in_the_model_three_sft_steps_and_the_swapped_forward(case):
    """Three ``sft_step(..., ema=ema)`` calls on the fwd_actions configuration.  The shadow equals ema_ref.update applied to the weights
    (``p``, ``lo``) recorded after each step, at the schedule's decays 0, 2/11, 3/12.  Then a forward under ``average_parameters()`` equals
    the forward of a fresh model that holds ``bf16(shadow)`` - launched eagerly and replayed by a ``GraphedTransformer`` that captured
    before the swap - and after ``restore()`` both give the pre-swap output again."""
    from orv_amd import FusedEMA, schedulers, sft
    from orv_amd.cogvideox_control import CogVideoXImageToVideoPipelineTraj as Pipe
    from orv_amd.optim import FusedAdamW
    g = _golden()
    lora = case.startswith("lora")
    precision = "bf16" if case == "all_bf16" else "split_fp32"
    sched = schedulers.CogVideoXDDIMScheduler(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012,
                                              beta_schedule="scaled_linear", prediction_type="v_prediction",
                                              rescale_betas_zero_snr=True, snr_shift_scale=3.0, timestep_spacing="trailing")
    x0 = torch.randn(2, 3, 16, 8, 12, generator=torch.Generator().manual_seed(9)).to(DEV, BF)
    batch = sft.Batch(x0, torch.zeros_like(x0), g["ins"]["encoder_hidden_states"].to(DEV, BF), g["ins"]["actions"].to(DEV), None, None,
                      torch.ones(3, dtype=torch.bool, device=DEV), 1)
    m = _fresh(g, lora).train()
    eval_mask = m.action_embed.forced_mask
    m.action_embed.forced_mask = torch.zeros(2, dtype=torch.bool)
    params = [p for p in m.parameters() if p.requires_grad]
    assert len(params) == (2 * 4 * g["cfg"]["num_layers"] if lora else len(list(m.parameters())))          # the adapter alone / everything
    opt = FusedAdamW(params, lr=1e-2 if lora else 2e-4, betas=(0.9, 0.95), weight_decay=1e-3, max_grad_norm=1.0, param_precision=precision)
    ema = FusedEMA(opt)
    f = opt._flat
    assert ema.shadow.numel() == f["p"].numel()
    want = ema.shadow.cpu().numpy().copy()
    assert np.array_equal(want.view(np.uint32), R.theta(*_flat_cpu(opt)).view(np.uint32))
    for step in range(1, 4):
        loss, parts = sft.sft_step(m, sched, opt, batch, generator=torch.Generator(device=DEV).manual_seed(100 + step), ema=ema)
        torch.cuda.synchronize()
        assert torch.isfinite(loss) and parts["grad_norm"] > 0 and ema.optimization_step == step
        assert ema.cur_decay_value == [0.0, 2 / 11, 3 / 12][step - 1]
        p_bits, lo = _flat_cpu(opt)
        want = R.update(want, p_bits, lo, R.omd_of(ema.cur_decay_value))
        got = _u32(ema.shadow)
        assert np.array_equal(got, want.view(np.uint32)), (step, np.flatnonzero(got != want.view(np.uint32))[:8])
    assert not np.array_equal(want.view(np.uint32), R.theta(p_bits, lo).view(np.uint32)), "the average equals the last weights"
    if precision == "split_fp32":
        assert lo.any()

    m.eval()
    m.action_embed.forced_mask = eval_mask
    pipe = Pipe(transformer=m).enable_hip_graph(True)
    args, _ = lora_ref.model_inputs(g["extra"], g["ins"], DEV)
    kw = dict(hidden_states=args[0], encoder_hidden_states=args[1], controls_or_guidances=args[2], timestep=args[3], return_dict=False)

    def replayed():
        outs = [pipe.transformer_forward(**kw)[0].clone() for _ in range(3)]       # eager warm-up, capture, replay
        torch.cuda.synchronize()
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
        return outs[2]
    before = _forward(m, g)
    assert torch.equal(replayed(), before)
    # the fresh model that holds bf16(shadow) in place of every trainable parameter (and the trained model's other weights)
    fresh = _fresh(g, lora)
    shadows = ema.shadow_tensors()
    with torch.no_grad():
        for (name, dst), (name2, src) in zip(fresh.named_parameters(), m.named_parameters()):
            assert name == name2
            dst.copy_(shadows[src].to(BF) if src in shadows else src)
    ref = _forward(fresh, g)
    assert not torch.equal(ref, before)
    with ema.average_parameters():
        assert torch.equal(_forward(m, g), ref), "eager forward on the swapped-in averages"
        assert torch.equal(replayed(), ref), "graph replay on the swapped-in averages"
    assert torch.equal(_forward(m, g), before), "eager forward after restore()"
    assert torch.equal(replayed(), before), "graph replay after restore()"
    p_after, lo_after = _flat_cpu(opt)
    assert np.array_equal(p_after, p_bits) and (lo is None or np.array_equal(lo_after, lo))


def test_state_dict_continues_bit_for_bit_and_a_permuted_list_is_refused():
    from orv_amd import FusedEMA
    from orv_amd.optim import FusedAdamW

    def feed(params, t):
        for i, p in enumerate(params):
            p.grad = (torch.randn(p.shape, generator=torch.Generator().manual_seed(1000 * t + i)) * 0.05).to(DEV, BF)

    def build(seed, order=slice(None)):
        gen = torch.Generator().manual_seed(seed)
        params = [torch.nn.Parameter((torch.randn(n, generator=gen) * 0.02).to(DEV, BF)) for n in SIZES][order]
        # no clipping: the clip coefficient comes from orv_sumsq, whose cross-workgroup float atomics add in arrival order, so with it two
        # runs of the OPTIMIZER differ in the last bits of the masters; the weights fed to both averages must be the same
        opt = FusedAdamW(params, lr=1e-2, max_grad_norm=0.0, param_precision="split_fp32")
        return params, opt, FusedEMA(opt, decay=0.9, use_ema_warmup=True)

    def run(steps, save_at=None):
        params, opt, ema = build(7)
        for t in range(1, steps + 1):
            if t == save_at:
                sd = {k: ([x.clone() for x in v] if k == "shadow_params" else v) for k, v in ema.state_dict().items()}
                osd = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in opt.state_dict().items()}
                weights = [p.detach().clone() for p in params]
                params, opt, _ = build(8)
                with torch.no_grad():
                    for p, w in zip(params, weights):
                        p.copy_(w)
                opt.load_state_dict(osd)
                ema = FusedEMA(opt)
                ema.load_state_dict(sd)
            feed(params, t)
            opt.step()
            opt.zero_grad()
            ema.step()
        torch.cuda.synchronize()
        return ema

    a, b = run(6), run(6, save_at=4)
    for x, y in zip(a.optimizer.master_params(), b.optimizer.master_params()):
        assert torch.equal(x, y), "the two optimizer runs differ: the averages were not fed the same weights"
    assert np.array_equal(_u32(a.shadow), _u32(b.shadow)) and a.optimization_step == b.optimization_step == 6
    assert _u32(a.shadow).any()
    _, _, permuted = build(7, order=slice(None, None, -1))
    with pytest.raises(ValueError, match="FusedEMA.load_state_dict: same parameters, another flat-buffer ORDER"):
        permuted.load_state_dict(a.state_dict())
