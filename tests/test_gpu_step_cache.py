"""GPU: the first-block step cache - the three kernels against the numpy restatement of the contract
(tests/step_cache_ref.py), the cached forward against the oracle's pieces, the decision, graph replay of the three segments, the
pipeline's policy."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import load_golden  # noqa: E402
import step_cache_ref as ref  # noqa: E402

BF = torch.bfloat16
INF = float("inf")
DEV = "cuda:0"

# (B, Nt, Nv, D).  A workgroup owns 1024 16-byte units (8192 values) of one clip, a lane four of them 256 units apart:
#   (1, 0, 1, 64): 8 units, one partly filled wave;  (3, 8, 72, 128): 1152 units, a second workgroup of 128 units;
#   (2, 226, 130, 1920): 31200 units = 30 full workgroups + 480 units;
#   (2, 3, 37, 576): 2664 units = 2 full workgroups + a ragged third of 616 units (2 x 256 + 104: lanes with three, two - and, in the last
#   waves, fewer - units), text rows in front, clips that start at no multiple of the workgroup's range.
SHAPES = [(1, 0, 1, 64), (3, 8, 72, 128), (2, 226, 130, 1920), (2, 3, 37, 576)]


def _inputs(B, Nt, Nv, D, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s, k=1.0: (torch.randn(*s, generator=g) * k).to(BF)
    # x0: joint buffer after iteration 0, xL: after the last one; e close to x0's video rows so that c is a small difference of large values
    x0 = r(B, Nt + Nv, D, k=3.0)
    e = (x0[:, Nt:].float() + torch.randn(B, Nv, D, generator=g) * 0.3).to(BF)
    p = r(B, Nv, D, k=0.3)
    xL = (x0.float() + torch.randn(B, Nt + Nv, D, generator=g)).to(BF)
    return x0, e, p, xL


def _run_kernels(x0, e, p, xL, B, Nt, Nv, D):
    """probe -> store -> apply on the device with NaN-poisoned outputs and scratch -> everything as numpy."""
    from orv_amd import ops
    nan = lambda *s, dt=BF: torch.full(s, float("nan"), dtype=dt, device=DEV)
    xd, ed, pd = x0.to(DEV), e.to(DEV), p.to(DEV)
    f, c, t = nan(B, Nv, D), nan(B, Nv, D), nan(B, Nv, D)
    sums = nan(B, 2, dt=torch.float64)
    scratch = nan(ops.step_cache_scratch(B, Nv, D), dt=torch.float64)
    x_before = xd.clone()
    ops.step_cache_probe(xd, ed, pd, f, c, sums, B, Nt, Nv, D, scratch=scratch)
    assert torch.equal(xd.view(torch.int16), x_before.view(torch.int16))          # the probe only reads x
    out = dict(f=ref.to_np(f), c=ref.to_np(c), sums=sums.cpu().numpy())
    ops.step_cache_store(xL.to(DEV), f, c, t, pd, B, Nt, Nv, D)
    out.update(t=ref.to_np(t), p=ref.to_np(pd))
    ya = xd.clone()
    ops.step_cache_apply(ya, t, B, Nt, Nv, D)
    out["applied"] = ref.to_np(ya)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernels_equal_the_restatement(shape):
    B, Nt, Nv, D = shape
    x0, e, p, xL = _inputs(B, Nt, Nv, D, seed=sum(shape))
    got = _run_kernels(x0, e, p, xL, B, Nt, Nv, D)
    f, c, sums = ref.probe_ref(ref.to_np(x0), ref.to_np(e), ref.to_np(p), Nt)
    t, p2 = ref.store_ref(ref.to_np(xL), f, c, Nt)
    applied = ref.apply_ref(ref.to_np(x0), t, Nt)
    for name, want in (("f", f), ("c", c), ("t", t), ("p", p2), ("applied", applied)):
        assert ref.same_bits(got[name], want), name
    assert ref.same_bits(got["applied"][:, :Nt], ref.to_np(x0)[:, :Nt])            # text rows untouched
    # fp64 addition of Nv * D non-negative terms in any order: relative error below Nv * D * 2^-53
    rel = np.abs(got["sums"] - sums) / sums
    print(f"[step-cache sums] {shape}: rel {rel.max():.2e} bound {Nv * D * 2.0 ** -53:.2e}")
    assert np.all(np.isfinite(got["sums"])) and rel.max() <= Nv * D * 2.0 ** -53
    again = _run_kernels(x0, e, p, xL, B, Nt, Nv, D)                               # two runs: the same bits, sums included
    for k in got:
        assert np.array_equal(got[k].view(np.uint64 if k == "sums" else np.uint32), again[k].view(np.uint64 if k == "sums" else np.uint32)), k


def test_nan_in_x_gives_nan_sums_and_only_for_its_clip():
    B, Nt, Nv, D = 3, 8, 72, 128
    x0, e, p, xL = _inputs(B, Nt, Nv, D, seed=5)
    x0[1, Nt + 70, 127] = float("nan")                 # the last workgroup of clip 1
    x0[2, 3, 5] = float("nan")                         # a TEXT row of clip 2: takes no part
    got = _run_kernels(x0, e, p, xL, B, Nt, Nv, D)
    _, _, sums = ref.probe_ref(ref.to_np(x0), ref.to_np(e), ref.to_np(p), Nt)
    assert np.isnan(sums[1, 0]) and np.isnan(got["sums"][1, 0])
    assert np.array_equal(np.isnan(got["sums"]), np.isnan(sums)) and np.isnan(got["sums"]).sum() == 1
    from orv_amd import step_cache as sc
    assert sc.decide(got["sums"].tolist(), INF)[0] is False                        # NaN computes


# ---- model and pipeline ----
def _build(cfg, w):
    from orv_amd.cogvideox_control import CogVideoXTransformer3DModelTraj
    m = CogVideoXTransformer3DModelTraj(**cfg)
    m.load_state_dict(w, strict=True)
    return m.to(DEV, BF).eval()


def _sched(name):
    from orv_amd import schedulers
    return getattr(schedulers, name)(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                                     clip_sample=False, set_alpha_to_one=True, prediction_type="v_prediction", rescale_betas_zero_snr=True,
                                     snr_shift_scale=3.0, timestep_spacing="trailing")


class _Loop:
    """A tiny pipeline on a ``pipe_*_bf16`` golden's model and inputs; ``run`` makes one call -> latents."""

    def __init__(self, name="pipe_ddim_bf16", graph=None):
        from orv_amd.cogvideox_control import CogVideoXImageToVideoPipelineTraj
        self.cfg, self.extra, self.ins, w, _ = load_golden(name)
        self.m = _build(self.cfg, w)
        self.m.action_embed.forced_mask = torch.zeros(self.ins["image"].shape[0], dtype=torch.bool)
        self.pipe = CogVideoXImageToVideoPipelineTraj(transformer=self.m, scheduler=_sched(self.extra["scheduler"]))
        if graph is not None:
            self.pipe.enable_hip_graph(graph)

    def run(self, steps, guidance=1.0, seed=11):
        ins = self.ins
        out = self.pipe(image=ins["image"].to(DEV, BF), height=64, width=96, num_frames=9, num_inference_steps=steps, guidance_scale=guidance,
                        generator=torch.Generator().manual_seed(seed), prompt_embeds=ins["prompt_embeds"].to(DEV, BF),
                        negative_prompt_embeds=ins["negative_prompt_embeds"].to(DEV, BF) if guidance > 1 else None, output_type="latent",
                        # under guidance the model's batch is doubled; like the reference's guided goldens those calls carry no actions
                        controls_or_guidances={"actions": ins["actions"].to(DEV, BF)} if guidance <= 1 else {})
        return out.frames.clone()


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("guidance", [1.0, 3.0])
@pytest.mark.parametrize("name", ["pipe_ddim_bf16", "pipe_dpm_bf16"])
def test_threshold_zero_never_skips_and_equals_the_uncached_loop(name, guidance, graph):
    lp = _Loop(name, graph)
    steps = lp.extra["steps"] + 2
    base = lp.run(steps, guidance)
    lp.pipe.enable_step_cache(0.0, compute_first=1, compute_last=0)
    got = lp.run(steps, guidance)
    rep = lp.pipe.step_cache_report
    assert len(rep) == steps and not any(r[2] for r in rep)
    assert [r[3] for r in rep] == ["first"] + ["threshold"] * (steps - 1)
    print(f"[step-cache report] {name} guidance {guidance} graph {graph}: {rep}")
    assert rep[0][1] is None and all(np.isfinite(r[1]) and r[1] > 0 for r in rep[1:])
    assert torch.equal(got.view(torch.int16), base.view(torch.int16))
    lp.pipe.disable_step_cache()
    assert torch.equal(lp.run(steps, guidance).view(torch.int16), base.view(torch.int16))      # off again == never enabled


def _rel_l2(got, want):
    got, want = got.float().cpu(), want.float().cpu()
    return ((got - want).norm() / want.norm()).item()


def _slice_rel_l2(got, want):
    """As tests/test_gpu_model.py: the largest rel-L2 over single frames and single channels of a [B, T, C, H, W] tensor."""
    got, want = got.float().cpu(), want.float().cpu()
    d = got - want
    per_frame = d.flatten(2).norm(dim=2) / want.flatten(2).norm(dim=2).clamp_min(1e-12)
    per_chan = d.transpose(1, 2).flatten(2).norm(dim=2) / want.transpose(1, 2).flatten(2).norm(dim=2).clamp_min(1e-12)
    return max(per_frame.max().item(), per_chan.max().item())


def _fwd_case(name):
    cfg, extra, ins, w, outs = load_golden(name)
    m = _build(cfg, w)
    m.action_embed.forced_mask = torch.tensor(extra["mask"])
    g = torch.Generator().manual_seed(7)
    hs_b = ins["hidden_states"] + 0.05 * torch.randn(ins["hidden_states"].shape, generator=g)      # perturbed latents,
    ts_b = ins["timestep"] - 40                                                                    # an earlier timestep
    assert int(ts_b.min()) >= 0

    def call(hs, ts):
        n = hs.shape[0]                                        # the first n clips of the golden's batch
        m.action_embed.forced_mask = torch.tensor(extra["mask"][:n])
        with torch.no_grad():
            return m(hs.to(DEV, BF), ins["encoder_hidden_states"][:n].to(DEV, BF), {"actions": ins["actions"][:n].to(DEV)}, ts.to(DEV),
                     return_dict=False, num_views=extra["num_views"])[0].clone()
    return cfg, extra, ins, w, m, hs_b, ts_b, call


@pytest.mark.parametrize("name", ["fwd_actions", "fwd_multiview"])
def test_skipped_forward_against_the_oracle_restatement(name):
    """Call A computed (bit-equal to the uncached forward), call B skipped: head(F_B + (X_A - F_A)) of the oracle in fp32, held to the
    bars tests/test_gpu_model.py holds these configs to (whole tensor 2e-2, worst frame / channel 4e-2)."""
    cfg, extra, ins, w, m, hs_b, ts_b, call = _fwd_case(name)
    plain_a, plain_b = call(ins["hidden_states"], ins["timestep"]), call(hs_b, ts_b)
    cache = m.enable_step_cache(INF)
    a = call(ins["hidden_states"], ins["timestep"])
    assert torch.equal(a.view(torch.int16), plain_a.view(torch.int16))
    assert [(h.skipped, h.reason) for h in cache.history] == [(False, "first")]
    b = call(hs_b, ts_b)
    rec = cache.history[-1]
    assert rec.skipped and rec.reason == "threshold" and np.isfinite(rec.max_distance) and len(rec.distances) == a.shape[0] * extra["num_views"]
    want, want_plain = ref.cached_forward_ref(w, cfg, ins, extra, hs_b, ts_b)
    e_c, w_c = _rel_l2(b, want), _slice_rel_l2(b, want)
    e_u, w_u = _rel_l2(plain_b, want_plain), _slice_rel_l2(plain_b, want_plain)
    print(f"[step-cache fwd] {name}: skipped B vs oracle restatement whole {e_c:.2e} worst {w_c:.2e} | uncached B vs oracle whole {e_u:.2e} "
          f"worst {w_u:.2e} | d = {rec.max_distance:.3e} | cached vs uncached B {_rel_l2(b, plain_b):.2e}")
    assert e_u <= 2e-2 and w_u <= 4e-2
    assert e_c <= 2e-2 and w_c <= 4e-2
    # the stored state is readable and is what the contract says: p of call A, F of call B
    assert cache.first_output.shape == cache.first_residual.shape == cache.tail_residual.shape
    assert tuple(cache.first_output.shape[1:]) == (72, 128)


def test_skipped_blocks_are_not_run():
    cfg, extra, ins, w, m, hs_b, ts_b, call = _fwd_case("fwd_actions")
    cache = m.enable_step_cache(INF)
    call(ins["hidden_states"], ins["timestep"])
    with torch.no_grad():
        for prm in m.transformer_blocks[1].parameters():
            prm.fill_(float("nan"))
    b = call(hs_b, ts_b)
    assert cache.history[-1].skipped and bool(torch.isfinite(b.float()).all())
    cache.force_compute()
    b2 = call(hs_b, ts_b)
    assert not cache.history[-1].skipped and cache.history[-1].reason == "forced"
    assert bool(torch.isnan(b2.float()).any())


def test_shape_change_invalidates_the_state():
    cfg, extra, ins, w, m, hs_b, ts_b, call = _fwd_case("fwd_actions")
    cache = m.enable_step_cache(INF)
    call(ins["hidden_states"], ins["timestep"])
    call(hs_b, ts_b)
    call(hs_b[:1], ts_b[:1])                                   # one clip: another shape
    call(hs_b[:1], ts_b[:1])
    call(hs_b, ts_b)                                           # back: the state belongs to the one-clip shape
    assert [(h.skipped, h.reason) for h in cache.history] == [(False, "first"), (True, "threshold"), (False, "shape"), (True, "threshold"),
                                                              (False, "shape")]


def test_data_dependent_decision():
    """tau is chosen from a threshold-0 run's distances, a factor 2 (>= 1.5) above the first distance that falls below it and a factor
    >= 1.5 below every earlier one: the run with tau computes every step before that one and skips it."""
    lp = _Loop("pipe_ddim_bf16", graph=False)
    steps = 8
    lp.pipe.enable_step_cache(0.0, compute_first=1, compute_last=0)
    lp.run(steps)
    d = [r[1] for r in lp.pipe.step_cache_report]
    print("[step-cache distances] " + " ".join("None" if v is None else f"{v:.3e}" for v in d))
    # the first step k >= 1 whose distance is at least a factor 3 below every earlier one: tau = 2 d_k is 1.5 away from all of d_1 .. d_k
    k = next((i for i in range(2, steps) if all(d[j] >= 3 * d[i] for j in range(1, i))), None)
    if k is None:                            # distances that do not fall: the first cached step is the one (nothing earlier to stay above)
        k = 1
    tau = 2 * d[k]
    assert all(d[j] >= 1.5 * tau for j in range(1, k)) and d[k] * 1.5 <= tau
    lp.pipe.enable_step_cache(tau, compute_first=1, compute_last=0)
    lp.run(steps)
    rep = lp.pipe.step_cache_report
    assert [r[2] for r in rep[:k + 1]] == [False] * k + [True], rep
    assert [r[1] for r in rep[1:k + 1]] == d[1:k + 1]          # the same distances, to the bit, up to the first skip


def test_data_dependent_decision_on_a_designed_sequence():
    """Six forwards whose latents take large random steps, except the fifth, which barely moves: its distance is far below the others.
    The threshold-0 run records the distances, tau = 2 d_4 lies a factor >= 1.5 from every distance up to there, and the run with tau
    computes forwards 0 .. 3 and skips forward 4."""
    cfg, extra, ins, w, m, _, _, call = _fwd_case("fwd_actions")
    g = torch.Generator().manual_seed(13)
    hs, seq = ins["hidden_states"], []
    for scale in (0.0, 0.5, 0.5, 0.5, 0.005, 0.5):
        hs = hs + scale * torch.randn(hs.shape, generator=g)
        seq.append(hs)
    ts = [ins["timestep"] - 30 * i for i in range(len(seq))]
    ts[4] = ts[3]                                              # the fifth forward: the fourth's timestep, latents a hair away

    def run(threshold):
        cache = m.enable_step_cache(threshold)
        for h, t in zip(seq, ts):
            call(h, t)
        return cache.history
    d = [h.max_distance for h in run(0.0)]
    print("[step-cache designed distances] " + " ".join("None" if v is None else f"{v:.3e}" for v in d))
    k = next(i for i in range(1, len(d)) if all(d[j] >= 3 * d[i] for j in range(1, i)) and i > 1)
    assert k == 4
    tau = 2 * d[k]
    assert all(d[j] >= 1.5 * tau for j in range(1, k)) and 1.5 * d[k] <= tau
    hist = run(tau)
    assert [h.skipped for h in hist[:k + 1]] == [False] * k + [True]
    assert [h.max_distance for h in hist[1:k + 1]] == d[1:k + 1]
    assert not hist[5].skipped and hist[5].reason == "threshold" and hist[5].max_distance >= 1.5 * tau      # and computes again after it


def test_graph_replay_of_all_three_segments_is_bit_identical():
    """8 steps, threshold inf, one skip at most in a row, the last step computed: C S C S C S C C - front replays from step 3 on, tail
    from step 5 (its third call), skip from step 6 (its third call)."""
    res = []
    for graph in (False, True):
        lp = _Loop("pipe_ddim_bf16", graph)
        lp.pipe.enable_step_cache(INF, max_consecutive_skips=1, compute_last=1)
        lat = lp.run(8)
        rep = lp.pipe.step_cache_report
        assert "".join("S" if r[2] else "C" for r in rep) == "CSCSCSCC"
        assert [r[3] for r in rep] == ["first", "threshold", "cap", "threshold", "cap", "threshold", "cap", "forced"]
        res.append((lat, rep))
        if graph:
            segs = sorted(k[-1] for k, st in lp.pipe._graphed._state.items() if "graph" in st)
            assert segs == ["front", "skip", "tail"], segs
    assert torch.equal(res[0][0].view(torch.int16), res[1][0].view(torch.int16))
    assert res[0][1] == res[1][1]


def test_policy_and_cold_start():
    lp = _Loop("pipe_ddim_bf16")
    lp.pipe.enable_step_cache(INF, compute_first=3, compute_last=2)
    first = lp.run(8)
    rep1 = lp.pipe.step_cache_report
    assert "".join("S" if r[2] else "C" for r in rep1) == "CCCSSSCC"
    assert [r[3] for r in rep1] == ["first", "forced", "forced", "threshold", "threshold", "threshold", "forced", "forced"]
    second = lp.run(8)                                         # a second call starts cold: the same report, the same latents
    assert lp.pipe.step_cache_report == rep1 and torch.equal(first.view(torch.int16), second.view(torch.int16))
    assert len(lp.m._step_cache.history) == 8


def test_rollout_with_the_cache_equals_the_hand_loop():
    """``pipe.rollout`` against the loop written by hand from the public pieces (the world of tests/test_gpu_rollout.py: three chunks of
    two steps), the cache on in both: every chunk starts cold, computes its first step and skips its second."""
    from test_gpu_rollout import World
    world = World()
    world.pipe.enable_step_cache(INF, compute_first=1, compute_last=0)
    want, _ = world.by_hand(0)
    rep = world.pipe.step_cache_report
    assert [(r[2], r[3]) for r in rep] == [(False, "first"), (True, "threshold")]          # the last chunk's report
    got = world.rolled([0]).frames[0].cpu().numpy()
    assert [(r[2], r[3]) for r in world.pipe.step_cache_report] == [(False, "first"), (True, "threshold")]
    assert np.array_equal(got, want)
    world.pipe.disable_step_cache()
    plain = world.by_hand(0, run=1)[0]
    assert not np.array_equal(plain, want)                     # the cache was really on: a skipped step changes the episode
