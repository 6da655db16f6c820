"""GPU: the snapshot kernels (``orv_snapshot``, ``orv_checksum``) against the numpy restatement of the checksum contract
(tests/train_state_ref.py), bit for bit, for the copy and for both sums; ``save_state`` / ``load_state`` resuming every fused optimizer bit
for bit on synthetic gradients; the snapshot being taken AT the save while training goes on; the model round trip with and without a LoRA
adapter; refusals and the device-side verification."""
import os

import numpy as np
import pytest
import torch

import lora_ref
import train_state_ref as R

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
DEV = torch.device("cuda:0")
GUARD = 0xA5


# ---- the kernels ----
def _layout(sizes_and_residues):
    """Byte offsets of the entries inside one buffer: at least 16 guard bytes in front of and behind each, start = residue mod 16."""
    offs, cur = [], 0
    for size, res in sizes_and_residues:
        start = (cur + 15) // 16 * 16 + 16 + res
        offs.append(start)
        cur = start + size + 16
    return offs, (cur + 15) // 16 * 16 + 16


def _run_table(cases, contents):
    """cases: [(bytes, src residue, dst residue)]; contents: per case the source bytes (numpy uint8).  One ``snapshot_into`` over the whole
    table, one ``checksum`` over the same sources; every copy, every guard byte and every pair is compared with the restatement."""
    from orv_amd import ops
    s_off, s_len = _layout([(n, rs) for n, rs, _ in cases])
    d_off, d_len = _layout([(n, rd) for n, _, rd in cases])
    src_h = np.full(s_len, 0x3C, dtype=np.uint8)
    for (n, _, _), o, c in zip(cases, s_off, contents):
        src_h[o:o + n] = c
    src = torch.from_numpy(src_h).to(DEV)
    dst = torch.full((d_len,), GUARD, dtype=torch.uint8, device=DEV)
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
    tensors = [src[o:o + n] for (n, _, _), o in zip(cases, s_off)]
    copies = [dst[o:o + n] for (n, _, _), o in zip(cases, d_off)]
    for (n, rs, rd), t, c in zip(cases, tensors, copies):
        assert n == 0 or (t.data_ptr() % 16 == rs and c.data_ptr() % 16 == rd)
    sums = ops.sums_to_ints(ops.snapshot_into(tensors, copies))
    only = ops.sums_to_ints(ops.checksum(tensors))
    torch.cuda.synchronize()
    dst_h = dst.cpu().numpy()
    want = np.full(d_len, GUARD, dtype=np.uint8)
    for (n, _, _), o, c in zip(cases, d_off, contents):
        want[o:o + n] = c
    bad = np.flatnonzero(dst_h != want)
    assert bad.size == 0, ("copy or guard bytes differ", bad[:8], dst_h[bad[:8]], want[bad[:8]])
    assert np.array_equal(src.cpu().numpy(), src_h), "the source was written"
    for i, ((n, rs, rd), c) in enumerate(zip(cases, contents)):
        ref = R.checksum_bytes(c.tobytes())
        assert sums[i] == ref, ("orv_snapshot", i, n, rs, rd, sums[i], ref)
        assert only[i] == ref, ("orv_checksum", i, n, rs, rd, only[i], ref)
    return sums


def test_kernels_equal_the_restatement_at_every_size_and_alignment():
    from orv_amd import ops
    C = ops.snapshot_chunk_bytes()
    sizes = [0, 1, 2, 3, 4, 5, 15, 16, 17, 4095, 4096, 4097, C - 4, C - 1, C, C + 1, C + 4, 3 * C + 5]
    cases = [(n, rs, rd) for n in sizes for rs in (0, 4, 8, 12) for rd in (0, 4, 8, 12)]
    rng = np.random.default_rng(0)
    contents = [rng.integers(0, 256, n, dtype=np.uint8) for n, _, _ in cases]
    cases.append((3 * C + 5, 4, 8))
    contents.append(np.full(3 * C + 5, 0xFF, dtype=np.uint8))                    # the largest words: s1 and s2 at their fastest growth
    sums = _run_table(cases, contents)
    assert sums[0] == (0, 0) and len(set(sums)) > len(sizes)


def test_tables_of_one_entry_and_of_a_thousand_small_ones():
    rng = np.random.default_rng(1)
    _run_table([(4097, 8, 4)], [rng.integers(0, 256, 4097, dtype=np.uint8)])
    _run_table([(0, 0, 0)], [np.zeros(0, dtype=np.uint8)])
    cases = [(6, 4 * (i % 4), 4 * ((i // 4) % 4)) for i in range(1000)]
    sums = _run_table(cases, [rng.integers(0, 256, 6, dtype=np.uint8) for _ in cases])
    assert len(set(sums)) > 990


def test_snapshot_allocates_copies_of_any_dtype_and_sums_without_copying():
    from orv_amd import ops
    g = torch.Generator().manual_seed(3)
    tensors = [torch.randn(2049, generator=g).to(DEV), torch.randn(3, 5, generator=g).to(DEV, BF), torch.zeros(0, device=DEV),
               torch.randint(-32768, 32768, (4101,), generator=g).to(DEV, torch.int16), torch.randn(7, generator=g).double().to(DEV)]
    copies, sums = ops.snapshot(tensors, copy=[True, True, True, False, True])
    sums = ops.sums_to_ints(sums)
    assert copies[3] is None
    for t, c, s in zip(tensors, copies, sums):
        assert s == R.checksum(t)
        if c is not None:
            assert c.dtype == t.dtype and c.shape == t.shape and (t.numel() == 0 or c.data_ptr() != t.data_ptr()) and R.tensor_bytes(c) == R.tensor_bytes(t)
    with pytest.raises(RuntimeError, match="must be contiguous"):
        ops.checksum([tensors[1].t()])
    with pytest.raises(RuntimeError, match="4-byte aligned address"):
        ops.checksum([tensors[1].view(-1)[1:]])


# ---- resume on synthetic gradients ----
class _Bag(torch.nn.Module):
    def __init__(self, params):
        super().__init__()
        self.w = torch.nn.ParameterList(params)


ADAMW_SIZES = [(1,), (2047,), (2049,)]                                           # tests/test_gpu_ema.py
PRODIGY_SIZES = [(4101,), (1,), (4096,), (2048,)]                                # tests/test_gpu_prodigy.py
CAME_SHAPES = [(3, 5), (130, 257), (1, 7), (7, 1), (5, 3, 2, 2), (2049,), (), (63, 255), (64, 256), (65, 257), (65, 264), (33, 65)]   # test_gpu_came.py

# no clipping anywhere: the clip coefficient comes from a sum of squares whose cross-workgroup order is not fixed (the existing resume tests)
OPTIMIZERS = {
    "adamw_bf16": (ADAMW_SIZES, lambda ps: _optim().FusedAdamW(ps, lr=1e-2, max_grad_norm=0.0)),
    "adamw_split_fp32": (ADAMW_SIZES, lambda ps: _optim().FusedAdamW(ps, lr=1e-2, max_grad_norm=0.0, param_precision="split_fp32")),
    "adamw_stochastic": (ADAMW_SIZES, lambda ps: _optim().FusedAdamW(ps, lr=1e-2, max_grad_norm=0.0, param_precision="stochastic", seed=17)),
    "adamw_fp8": (ADAMW_SIZES, lambda ps: _optim().FusedAdamW(ps, lr=1e-2, max_grad_norm=0.0, state_precision="fp8", seed=5)),
    "prodigy": (PRODIGY_SIZES, lambda ps: _optim().FusedProdigy(ps, lr=1.0, betas=(0.9, 0.95), max_grad_norm=0.0)),
    "came": (CAME_SHAPES, lambda ps: _optim().FusedCAME(ps, 1e-3, weight_decay=1e-2, max_grad_norm=0.0, param_precision="split_fp32")),
}
NOT_STATE = {"g", "g_params", "g_mask", "active", "seg_start", "partials", "came_scratch", "came_geom"}


def _optim():
    from orv_amd import optim
    return optim


class _Run:
    """Parameters, optimizer, EMA, schedule and generator of one run; ``seed`` sets the initial weights and the generator."""

    def __init__(self, kind, seed):
        from orv_amd import FusedEMA
        shapes, make = OPTIMIZERS[kind]
        gen = torch.Generator().manual_seed(seed)
        self.params = [torch.nn.Parameter((torch.randn(s, generator=gen) * 0.02).to(DEV, BF)) for s in shapes]
        self.bag = _Bag(self.params)
        self.opt = make(self.params)
        self.ema = FusedEMA(self.opt, decay=0.9, use_ema_warmup=True)
        self.sched = _optim().get_scheduler("cosine_with_restarts", self.opt, num_warmup_steps=1, num_training_steps=20)
        self.gen = torch.Generator(device=DEV).manual_seed(seed)
        self.kw = dict(model=self.bag, optimizer=self.opt, lr_scheduler=self.sched, ema=self.ema, generator=self.gen)

    def steps(self, first, last):
        for t in range(first, last + 1):
            for i, p in enumerate(self.params):
                p.grad = (torch.randn(p.shape, generator=torch.Generator().manual_seed(1000 * t + i)) * 0.05).to(DEV, BF)
            torch.randn(5, generator=self.gen, device=DEV)                   # the loop draws its noise from the generator
            self.opt.step()
            self.opt.zero_grad()
            self.ema.step()
            self.sched.step()
        torch.cuda.synchronize()
        return self

    def state(self):
        """Every buffer that is state, as bytes, plus the host scalars."""
        f = self.opt._flat
        out = {k: R.tensor_bytes(v) for k, v in f.items() if torch.is_tensor(v) and k not in NOT_STATE}
        out.update({"came_" + k: R.tensor_bytes(v) for k, v in f.get("came_stats", {}).items() if v is not None})
        out["shadow"] = R.tensor_bytes(self.ema.shadow)
        out["host"] = (self.opt.step_count, self.opt.seed, self.opt.param_groups[0]["lr"], self.sched.last_epoch, self.ema.optimization_step,
                       self.ema.decay, self.ema.use_ema_warmup)
        return out

    def next_draw(self):
        return R.tensor_bytes(torch.randn(8, generator=self.gen, device=DEV))


@pytest.mark.parametrize("kind", list(OPTIMIZERS))
def test_resume_is_bit_identical(kind, tmp_path):
    """6 steps straight against 3 steps, ``save_state``, fresh objects (other initial weights, other generator seed), ``load_state``, 3 steps."""
    from orv_amd import load_state, save_state
    straight = _Run(kind, 7).steps(1, 6)
    first = _Run(kind, 7).steps(1, 3)
    handle = save_state(str(tmp_path), 3, extra={"epoch": 2}, **first.kw)
    assert handle.path == str(tmp_path / "checkpoint-3")
    handle.wait()
    assert handle.done and sorted(os.listdir(tmp_path)) == ["checkpoint-3"]
    assert sorted(os.listdir(handle.path)) == ["ema.json", "ema.safetensors", "manifest.json", "optimizer.json", "optimizer.safetensors",
                                               "random_states.json", "scheduler.json", "transformer"]
    second = _Run(kind, 8)
    assert second.state()["p"] != first.state()["p"]
    where = [p.data_ptr() for p in second.params]
    info = load_state(str(tmp_path), resume="latest", **second.kw)
    assert info == {"step": 3, "extra": {"epoch": 2}}
    assert [p.data_ptr() for p in second.params] == where, "a parameter left its storage"
    at_save, loaded = first.state(), second.state()
    assert sorted(at_save) == sorted(loaded) and all(at_save[k] == loaded[k] for k in at_save), [k for k in at_save if at_save[k] != loaded[k]]
    second.steps(4, 6)
    a, b = straight.state(), second.state()
    keys = {"p", "seg_step", "shadow", "host"} | {"adamw_bf16": {"m", "v"}, "adamw_split_fp32": {"m", "v", "lo"}, "adamw_stochastic": {"m", "v"},
                                                 "adamw_fp8": {"m8", "v8", "m_exp", "v_exp"}, "prodigy": {"m", "v", "lo", "s", "p0", "pstate"},
                                                 "came": {"m", "lo", "came_r", "came_c", "came_res_r", "came_res_c", "came_v"}}[kind]
    assert keys <= set(a), keys - set(a)
    assert sorted(a) == sorted(b) and all(a[k] == b[k] for k in a), [k for k in a if a[k] != b[k]]
    assert a["p"] != at_save["p"] and a["shadow"] != at_save["shadow"] and any(a["shadow"])
    assert straight.next_draw() == second.next_draw()


def test_the_snapshot_is_taken_at_the_save_and_both_modes_write_the_same_bytes(tmp_path):
    from orv_amd import load_state, save_state
    run = _Run("adamw_split_fp32", 7).steps(1, 3)
    at_save = run.state()
    draw_state = run.gen.get_state()
    blocking = save_state(str(tmp_path / "a"), 3, blocking=True, **run.kw)
    assert blocking.done and os.path.exists(os.path.join(blocking.path, "manifest.json"))
    handle = save_state(str(tmp_path / "b"), 3, blocking=False, **run.kw)
    run.steps(4, 5)                                   # at once: the writer has the copies, the loop has the buffers
    handle.wait()
    now = run.state()
    assert now["p"] != at_save["p"] and now["m"] != at_save["m"] and now["shadow"] != at_save["shadow"]
    a, b = R.tree_bytes(blocking.path), R.tree_bytes(handle.path)
    assert sorted(a) == sorted(b) and all(a[k] == b[k] for k in a), [k for k in a if a[k] != b[k]]
    fresh = _Run("adamw_split_fp32", 8)
    load_state(handle.path, **fresh.kw)
    got = fresh.state()
    assert all(got[k] == at_save[k] for k in at_save), [k for k in at_save if got[k] != at_save[k]]
    assert any(got[k] != now[k] for k in now)
    assert torch.equal(fresh.gen.get_state(), draw_state)
    assert not os.path.exists(tmp_path / "b" / ".tmp-checkpoint-3")


def test_rotation_after_the_save_and_latest(tmp_path):
    from orv_amd import latest_checkpoint, save_state
    run = _Run("adamw_bf16", 7).steps(1, 1)
    for step in (9, 10, 11):
        save_state(str(tmp_path), step, total_limit=2, **run.kw)          # each call waits for the one before
    save_state(str(tmp_path), 12, total_limit=2, blocking=True, **run.kw)
    assert sorted(os.listdir(tmp_path)) == ["checkpoint-11", "checkpoint-12"]
    assert latest_checkpoint(str(tmp_path)) == str(tmp_path / "checkpoint-12")


# ---- refusals and verification ----
def test_refusals_and_the_device_side_verification(tmp_path):
    from orv_amd import load_state, save_state
    run = _Run("adamw_bf16", 7).steps(1, 2)
    run.ema.store()
    with pytest.raises(RuntimeError, match=r"save_state: the averaged weights are swapped in"):
        save_state(str(tmp_path), 2, **run.kw)
    run.ema.restore()
    cpu = [torch.nn.Parameter(torch.zeros(5, dtype=BF))]
    with pytest.raises(RuntimeError, match=r"save_state: \d+ CPU tensors"):
        save_state(str(tmp_path), 2, model=_Bag(cpu), optimizer=_optim().FusedAdamW(cpu))
    stranger = [torch.nn.Parameter(torch.zeros(5, dtype=BF, device=DEV))]
    with pytest.raises(RuntimeError, match=r"optimizer.params\[0\] is not a trainable parameter of `model`"):
        save_state(str(tmp_path), 2, model=run.bag, optimizer=_optim().FusedAdamW(stranger))
    assert os.listdir(tmp_path) == []
    path = save_state(str(tmp_path), 2, blocking=True, **run.kw).path
    # another optimizer class: its own load_state_dict refuses
    other = [torch.nn.Parameter(torch.zeros(s, dtype=BF, device=DEV)) for s in ADAMW_SIZES]
    with pytest.raises(ValueError, match=r"FusedCAME.load_state_dict: the checkpoint was written by the 'adamw' optimizer"):
        load_state(path, model=_Bag(other), optimizer=_optim().FusedCAME(other, 1e-3))
    # another trainable set
    fewer = [torch.nn.Parameter(torch.zeros(s, dtype=BF, device=DEV)) for s in ADAMW_SIZES[:2]]
    with pytest.raises(RuntimeError, match="Unexpected key"):
        load_state(path, model=_Bag(fewer), optimizer=_optim().FusedAdamW(fewer))
    # one flipped bit in a moment, in a weight and in a shadow: found on the device, named
    for rel, name in (("optimizer.safetensors", "exp_avg_sq"), ("transformer/diffusion_pytorch_model.safetensors", "w.2"),
                      ("ema.safetensors", "shadow_params.1")):
        R.flip_byte_of(os.path.join(path, rel), name, at=7)
        fresh = _Run("adamw_bf16", 8)
        with pytest.raises(ValueError, match=rf"{os.path.dirname(rel) or rel}.*tensor '{name}' has checksum .* on the device"):
            load_state(path, **fresh.kw)
        load_state(path, verify=False, **_Run("adamw_bf16", 8).kw)
        R.flip_byte_of(os.path.join(path, rel), name, at=7)
    fresh = _Run("adamw_bf16", 8)
    load_state(path, **fresh.kw)
    assert fresh.state() == run.state()


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


@pytest.mark.parametrize("lora", [False, True], ids=["all_parameters", "lora_r16"])
def test_in_the_model_two_sft_steps_save_and_load_into_a_fresh_model(lora, tmp_path):
    from orv_amd import FusedEMA, load_state, save_state, schedulers, sft
    from orv_amd.cogvideox_control import CogVideoXTransformer3DModelTraj
    from orv_amd.optim import FusedAdamW, get_scheduler
    g = _golden()
    sched = schedulers.CogVideoXDDIMScheduler(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012,
                                              beta_schedule="scaled_linear", prediction_type="v_prediction",
                                              rescale_betas_zero_snr=True, snr_shift_scale=3.0, timestep_spacing="trailing")
    x0 = torch.randn(2, 3, 16, 8, 12, generator=torch.Generator().manual_seed(9)).to(DEV, BF)
    batch = sft.Batch(x0, torch.zeros_like(x0), g["ins"]["encoder_hidden_states"].to(DEV, BF), g["ins"]["actions"].to(DEV), None, None,
                      torch.ones(3, dtype=torch.bool, device=DEV), 1)

    def build():
        m = _fresh(g, lora)
        opt = FusedAdamW([p for p in m.parameters() if p.requires_grad], lr=1e-2 if lora else 2e-4, betas=(0.9, 0.95), weight_decay=1e-3,
                         param_precision="split_fp32")
        return m, opt, FusedEMA(opt), get_scheduler("constant_with_warmup", opt, num_warmup_steps=0)

    m, opt, ema, lrs = build()
    m.train()
    eval_mask = m.action_embed.forced_mask
    m.action_embed.forced_mask = torch.zeros(2, dtype=torch.bool)
    gen = torch.Generator(device=DEV).manual_seed(100)
    for _ in range(2):
        loss, parts = sft.sft_step(m, sched, opt, batch, generator=gen, lr_scheduler=lrs, ema=ema)
        assert torch.isfinite(loss) and parts["grad_norm"] > 0
    m.eval()
    m.action_embed.forced_mask = eval_mask
    before = _forward(m, g)
    path = save_state(str(tmp_path), 2, model=m, optimizer=opt, lr_scheduler=lrs, ema=ema, generator=gen, blocking=True).path
    if lora:
        assert os.path.exists(os.path.join(path, lora_ref.FILE_NAME)) and not os.path.exists(os.path.join(path, "transformer"))
    else:
        assert sorted(os.listdir(os.path.join(path, "transformer"))) == ["config.json", "diffusion_pytorch_model.safetensors"]
        again = CogVideoXTransformer3DModelTraj.from_pretrained(os.path.join(path, "transformer"), torch_dtype=BF)
        for (k, a), (k2, b) in zip(again.state_dict().items(), m.state_dict().items()):
            assert k == k2 and R.tensor_bytes(a) == R.tensor_bytes(b), k
    m2, opt2, ema2, lrs2 = build()
    gen2 = torch.Generator(device=DEV).manual_seed(1)
    assert not torch.equal(_forward(m2, g), before)
    assert load_state(path, model=m2, optimizer=opt2, lr_scheduler=lrs2, ema=ema2, generator=gen2)["step"] == 2
    for (k, a), (k2, b) in zip(m2.state_dict().items(), m.state_dict().items()):
        assert k == k2 and R.tensor_bytes(a) == R.tensor_bytes(b), k
    if lora:
        for (k, a), b in zip(m2.get_adapter_state_dict().items(), m.get_adapter_state_dict().values()):
            assert R.tensor_bytes(a) == R.tensor_bytes(b) and bool(a.any()), k
    f, f2 = opt._flat, opt2._flat
    for k in ("p", "lo", "m", "v", "seg_step"):
        assert R.tensor_bytes(f[k]) == R.tensor_bytes(f2[k]), k
    assert bool(f2["lo"].any()) and bool(f2["m"].any())
    assert R.tensor_bytes(ema.shadow) == R.tensor_bytes(ema2.shadow) and ema2.optimization_step == 2 and opt2.step_count == 2
    assert torch.equal(gen.get_state(), gen2.get_state()) and lrs2.last_epoch == lrs.last_epoch
    assert torch.equal(_forward(m2, g), before), "the inference forward of the loaded model"
