"""CPU restatement of the fused Prodigy optimizer (``orv_amd.optim.FusedProdigy``, include/orv_mi355.h ``orv_prodigy_*``), written from the
rule in DESIGN.md 4.3.3 and not from the kernels.  Not a test.

The rule restates ``prodigyopt`` 1.0's ``Prodigy.step`` FROM MEMORY: the package cannot be installed where this project is developed, so
nothing here was compared against it (UNPINNED, like the diffusers leaves of oracle/leaf.py).  ``slice_p`` and ``fsdp_in_use`` of newer
versions are not part of it; there is one parameter group.  The structure is ``prodigyopt``'s: a loop over the parameters that updates the
moments and gathers the two global sums, the scalar recurrence of the step-size estimate d in Python floats, a second loop that moves the
weights.

    bc  = sqrt(1 - b2^(k+1)) / (1 - b1^(k+1))  if use_bias_correction else 1
    dlr = d lr bc                                       (the OLD d, fixed for the whole step)
    num = beta3 d_numerator
    per element of a parameter with a gradient:   p0 = w at its first update;  g += wd w (coupled decay only)
        num += ((d / d0) dlr g) (p0 - w) ;  m = b1 m + (d (1 - b1)) g ;  v = b2 v + ((d d (1 - b2)) g) g
        s = beta3 s + ((d / d0) (d if safeguard_warmup else dlr)) g ;  den += |s|
    den == 0: return (m, v, s stay written; d, d_max, d_numerator, k and every weight stay)
    d_hat = d_coef num / den ;  if d == d0: d = max(d, d_hat) ;  d_max = max(d_max, d_hat) ;  d = min(d_max, d growth_rate) ;  d_numerator = num
    per element:   w -= (wd dlr) w (decoupled decay only) ;  w -= (dlr m) / (sqrt(v) + d eps)        (the NEW d, the old dlr)
    k += 1

``dtype`` chooses the evaluation: ``torch.float32`` rounds every operation separately in the kernels' order - the hyper-parameters enter as
fp32 (the C ABI takes floats), the scalars d, dlr, d / d0 are Python floats (the device keeps them in fp64) that are rounded to fp32 where
they meet an element, and the two sums are formed per 2048-element chunk in fp32 in the kernel's fixed order (8 elements of a lane in
sequence, a balanced tree over the 64 lanes of a wave, the four waves in sequence) and across chunks in fp64.  ``torch.float64`` is the
yardstick: the same inputs, everything in double.

The weights are an fp32 master (``adamw_ref.split`` / ``rebuild`` define its storage as bf16 + int16); p0 is the bf16 part of the master at
the first update.  ``weights_mode="bf16"`` rounds the weights to bf16 after every update instead: the variant that shows why Prodigy needs the
master (updates of the size of d0 vanish, p0 - w stays 0, d never leaves d0).

``prodigy_moments`` / ``prodigy_recurrence`` / ``prodigy_update`` are stand-ins with the signatures of the ``orv_amd.ops`` wrappers on CPU
tensors, for CPU tests of the optimizer's host logic (as ``adamw_ref.adamw_flat_ex`` serves ``FusedAdamW``)."""
import math

import torch

import adamw_ref

SEG = 2048
STATE = ("d", "d_max", "d_numerator", "d_denom", "d_hat", "k", "dlr", "skip")       # the fp64[8] device state
DEFAULTS = dict(lr=1.0, betas=(0.9, 0.999), beta3=None, eps=1e-8, weight_decay=0.0, decouple=True, use_bias_correction=False,
                safeguard_warmup=False, d0=1e-6, d_coef=1.0, growth_rate=float("inf"))


def f32(x) -> float:
    """A Python float rounded to fp32 (what a ``float`` argument of the C ABI, or a scalar meeting an fp32 element, holds)."""
    return float(torch.tensor(float(x), dtype=torch.float32))


def new_scalars(d0=1e-6):
    return dict(d=float(d0), d_max=float(d0), d_numerator=0.0, d_denom=0.0, d_hat=0.0, k=0, dlr=0.0, skip=0)


def new_param_state(w):
    z = lambda: torch.zeros_like(w)
    return dict(m=z(), v=z(), s=z(), p0=None)


def step_dlr(sc, lr, b1, b2, use_bias_correction):
    """dlr = d lr bc from the scalars BEFORE the step (Python floats, i.e. fp64); lr, b1, b2 already rounded to fp32."""
    bc = 1.0
    if use_bias_correction:
        bc = math.sqrt(1.0 - b2 ** (sc["k"] + 1)) / (1.0 - b1 ** (sc["k"] + 1))
    return sc["d"] * lr * bc


def chunk_sums(x, dtype):
    """Sum of the per-element terms ``x`` (1-D, ``dtype``) over each chunk of 2048 (zero padded) -> float64 [chunks], in the kernel's order
    for fp32: ((((0 + t0) + t1) ...) + t7) per lane, a balanced adjacent-pairs tree over each wave's 64 lanes, ((w0 + w1) + w2) + w3."""
    n = x.numel()
    pad = (-n) % SEG
    if pad:
        x = torch.cat([x, torch.zeros(pad, dtype=x.dtype)])
    if dtype == torch.float64:
        return x.view(-1, SEG).sum(1)
    t = x.view(-1, 256, 8)
    lane = torch.zeros_like(t[..., 0])
    for e in range(8):
        lane = lane + t[..., e]
    w = lane.view(-1, 4, 64)
    while w.shape[-1] > 1:
        w = w[..., 0::2] + w[..., 1::2]
    w = w[..., 0]
    return (((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]).double()


def moments_(w, g, st, d, dlr, dtype, b1, b2, b3, wd, decouple, safeguard_warmup, d0, clip=1.0):
    """First loop body for one parameter: updates st["m"], st["v"], st["s"] in place -> (numerator terms, |s|) per element in ``dtype``.
    ``w`` the master, ``g`` the raw gradient (bf16 values), both given in ``dtype``; b1, b2, b3, wd, clip already fp32-rounded floats."""
    T = lambda x: torch.tensor(float(x), dtype=dtype)          # fp32: the scalar is rounded to fp32 where it meets an element
    one = torch.ones((), dtype=dtype)
    ratio = d / d0
    c_num, c_m, c_v = T(ratio * dlr), T(d) * (one - T(b1)), T(d) * T(d) * (one - T(b2))
    c_s = T(ratio * (d if safeguard_warmup else dlr))
    gr = g * T(clip)
    if wd != 0 and not decouple:
        gr = gr + T(wd) * w
    terms = (c_num * gr) * (st["p0"] - w)
    st["m"] = T(b1) * st["m"] + c_m * gr
    st["v"] = T(b2) * st["v"] + (c_v * gr) * gr
    st["s"] = T(b3) * st["s"] + c_s * gr
    return terms, st["s"].abs()


def recurrence_(sc, num_sum, den, dlr, b3, d0, d_coef, growth_rate):
    """The scalar recurrence in Python floats; ``num_sum`` is this step's sum alone.  -> True when the step is skipped (den == 0)."""
    sc["dlr"], sc["d_denom"] = dlr, den
    if den == 0.0:
        sc["skip"] = 1
        return True
    num = b3 * sc["d_numerator"] + num_sum
    d_hat = d_coef * num / den
    d = sc["d"]
    if d == d0:
        d = max(d, d_hat)
    sc["d_max"] = max(sc["d_max"], d_hat)
    sc["d"] = min(sc["d_max"], d * growth_rate)
    sc["d_numerator"], sc["d_hat"], sc["k"], sc["skip"] = num, d_hat, sc["k"] + 1, 0
    return False


def update_(w, st, d_new, dlr, dtype, eps, wd, decouple):
    """Second loop body for one parameter -> the new master in ``dtype``."""
    T = lambda x: torch.tensor(float(x), dtype=dtype)
    dn, dl = T(d_new), T(dlr)
    if wd != 0 and decouple:
        w = w - (T(wd) * dl) * w
    return w - (dl * st["m"]) / (torch.sqrt(st["v"]) + dn * T(eps))


def capture_p0(w, dtype):
    """p0 at a parameter's first update: the bf16 part of the fp32 master (the master itself when its low half is zero)."""
    return adamw_ref.split(w.float())[0].to(dtype)


def step(weights, grads, states, sc, dtype, clip=1.0, weights_mode="master", **hyper):
    """One Prodigy step over a list of parameters, in place on the lists ``weights`` (masters in ``dtype``; bf16 VALUES in ``dtype`` under
    ``weights_mode="bf16"``), ``states`` (``new_param_state``) and the dict ``sc`` (``new_scalars``).  ``grads[i]`` None: parameter i is
    skipped in both loops.  -> (this step's numerator sum, denominator)."""
    h = dict(DEFAULTS, **hyper)
    b1, b2 = f32(h["betas"][0]), f32(h["betas"][1])
    b3 = f32(math.sqrt(h["betas"][1]) if h["beta3"] is None else h["beta3"])
    lr, eps, wd, clip = f32(h["lr"]), f32(h["eps"]), f32(h["weight_decay"]), f32(clip)
    d, d0 = sc["d"], float(h["d0"])
    dlr = step_dlr(sc, lr, b1, b2, h["use_bias_correction"])
    num_sum, den = 0.0, 0.0
    for i, (w, g) in enumerate(zip(weights, grads)):
        if g is None:
            continue
        st = states[i]
        if st["p0"] is None:
            st["p0"] = capture_p0(w, dtype) if weights_mode == "master" else w.clone()
        terms, abs_s = moments_(w, g.to(dtype), st, d, dlr, dtype, b1, b2, b3, wd, h["decouple"], h["safeguard_warmup"], d0, clip)
        for c in chunk_sums(terms.reshape(-1), dtype).tolist():
            num_sum += c
        for c in chunk_sums(abs_s.reshape(-1), dtype).tolist():
            den += c
    if recurrence_(sc, num_sum, den, dlr, b3, d0, float(h["d_coef"]), float(h["growth_rate"])):
        return num_sum, den
    for i, (w, g) in enumerate(zip(weights, grads)):
        if g is None:
            continue
        w_new = update_(w, states[i], sc["d"], dlr, dtype, eps, wd, h["decouple"])
        weights[i] = w_new.to(torch.bfloat16).to(dtype) if weights_mode == "bf16" else w_new
    return num_sum, den


# ---- the experiment of DESIGN.md 4.3.3: why the fp32 master is not optional ----
def quadratic_problem(n=4096, seed=0):
    """-> (bf16 start weights N(0, 0.02^2), fp32 target N(0, 0.02^2)); the loss is 1/2 |w - target|^2, its gradient w - target."""
    gen = torch.Generator().manual_seed(seed)
    p = (torch.randn(n, generator=gen) * 0.02).to(torch.bfloat16)
    target = torch.randn(n, generator=gen) * 0.02
    return p, target


def quadratic_run(dtype=torch.float64, weights_mode="master", steps=60, betas=(0.9, 0.95), **hyper):
    """``steps`` Prodigy steps on the quadratic problem, gradients rounded to bf16 -> (d after every step, mean (w - target)^2 at the end)."""
    p, target = quadratic_problem()
    weights, states, sc = [p.to(dtype)], [new_param_state(p.to(dtype))], new_scalars(hyper.get("d0", 1e-6))
    hist = []
    for _ in range(steps):
        g = (weights[0] - target.to(dtype)).to(torch.bfloat16)
        step(weights, [g], states, sc, dtype, weights_mode=weights_mode, betas=betas, **hyper)
        hist.append(sc["d"])
    return hist, float(((weights[0].double() - target.double()) ** 2).mean())


# ---- flat layout: one step over segments (the GPU tests' reference) and the ops stand-ins ----
def _segments(seg_start, seg_active):
    starts = [int(x) for x in seg_start.tolist()]
    return [(i, starts[i], starts[i + 1]) for i in range(len(starts) - 1) if int(seg_active[i])]


def state_tensor(sc):
    return torch.tensor([float(sc[k]) for k in STATE], dtype=torch.float64)


def scalars_of(state):
    sc = dict(zip(STATE, [float(x) for x in state.tolist()]))
    sc["k"], sc["skip"] = int(sc["k"]), int(sc["skip"])
    return sc


def flat_step(w, g, p0, m, v, s, seg_start, seg_active, seg_step, sc, dtype, clip=1.0, **hyper):
    """One step on flat buffers (``w`` the fp32 master, ``p0`` bf16, ``seg_step`` the counts INCLUDING this step) evaluated in ``dtype``
    -> (w, p0, m, v, s) new tensors in ``dtype`` (p0 bf16), num_sum, den; ``sc`` is advanced in place.  Inactive segments keep everything."""
    segs = _segments(seg_start, seg_active)
    weights = [w[a:b].to(dtype) for _, a, b in segs]
    states = []
    for i, a, b in segs:
        first = int(seg_step[i]) == 1
        states.append(dict(m=m[a:b].to(dtype), v=v[a:b].to(dtype), s=s[a:b].to(dtype), p0=None if first else p0[a:b].to(dtype)))
    num_sum, den = step(weights, [g[a:b] for _, a, b in segs], states, sc, dtype, clip=clip, **hyper)
    out = [x.to(dtype).clone() for x in (w, m, v, s)]
    p0_new = p0.clone()
    for (i, a, b), wn, st in zip(segs, weights, states):
        out[0][a:b], out[1][a:b], out[2][a:b], out[3][a:b] = wn, st["m"], st["v"], st["s"]
        p0_new[a:b] = st["p0"].to(torch.bfloat16)
    return out[0], p0_new, out[1], out[2], out[3], num_sum, den


def prodigy_moments(p, lo, g, p0, m, v, s, seg_start, seg_active, seg_step, state, partials, lr, beta1, beta2, beta3, weight_decay=0.0,
                    decouple=True, safeguard_warmup=False, use_bias_correction=False, d0=1e-6, clip_coef=None):
    """Stand-in for ``orv_amd.ops.prodigy_moments`` on CPU tensors (fp32 arithmetic), in place."""
    assert p.numel() % SEG == 0 and partials.numel() * 1024 == p.numel() and state.numel() == len(STATE)
    sc = scalars_of(state)
    b1, b2, b3, lr, wd = f32(beta1), f32(beta2), f32(beta3), f32(lr), f32(weight_decay)
    clip = f32(float(clip_coef)) if clip_coef is not None else 1.0
    dlr = step_dlr(sc, lr, b1, b2, use_bias_correction)
    w = adamw_ref.rebuild(p, lo)
    partials.zero_()
    for i, a, b in _segments(seg_start, seg_active):
        if int(seg_step[i]) == 1:
            p0[a:b] = p[a:b]
        st = dict(m=m[a:b].clone(), v=v[a:b].clone(), s=s[a:b].clone(), p0=p0[a:b].float())
        terms, abs_s = moments_(w[a:b], g[a:b].float(), st, sc["d"], dlr, torch.float32, b1, b2, b3, wd, decouple, safeguard_warmup, float(d0), clip)
        m[a:b], v[a:b], s[a:b] = st["m"], st["v"], st["s"]
        partials[2 * (a // SEG):2 * (b // SEG):2] = chunk_sums(terms, torch.float32)
        partials[2 * (a // SEG) + 1:2 * (b // SEG):2] = chunk_sums(abs_s, torch.float32)


def prodigy_recurrence(state, partials, lr, beta1, beta2, beta3, use_bias_correction=False, d0=1e-6, d_coef=1.0, growth_rate=float("inf")):
    """Stand-in for ``orv_amd.ops.prodigy_recurrence``."""
    sc = scalars_of(state)
    dlr = step_dlr(sc, f32(lr), f32(beta1), f32(beta2), use_bias_correction)
    recurrence_(sc, sum(partials[0::2].tolist()), sum(partials[1::2].tolist()), dlr, f32(beta3), float(d0), float(d_coef), float(growth_rate))
    state.copy_(state_tensor(sc))


def prodigy_update(p, lo, m, v, seg_start, seg_active, state, eps, weight_decay=0.0, decouple=True):
    """Stand-in for ``orv_amd.ops.prodigy_update``."""
    assert eps > 0
    sc = scalars_of(state)
    if sc["skip"]:
        return
    w = adamw_ref.rebuild(p, lo)
    for _, a, b in _segments(seg_start, seg_active):
        w_new = update_(w[a:b], dict(m=m[a:b], v=v[a:b]), sc["d"], sc["dlr"], torch.float32, f32(eps), f32(weight_decay), decouple)
        p[a:b], lo[a:b] = adamw_ref.split(w_new)
