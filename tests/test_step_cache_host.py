"""CPU: the host side of the first-block step cache - the arithmetic of the contract on hand-derived values, the
``decide`` table, argument refusals of the C ABI and of the Python surface, header / ctypes agreement, the default state."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
import step_cache_ref as ref

from orv_amd import step_cache as sc

INF, NAN = float("inf"), float("nan")


def test_bf16_rounding_of_the_restatement_is_nearest_even():
    # 1 + 2^-8 lies exactly between the bf16 neighbours 1 and 1 + 2^-7: the tie goes to the even mantissa (1); 1 + 3 * 2^-8 to 1 + 2^-6
    a = np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -1.0 - 2.0 ** -8, 0.0, 3.0e38], dtype=np.float32)
    want = np.array([1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -1.0, 0.0, 3.0e38], dtype=np.float32)
    want[5] = torch.tensor(3.0e38).to(torch.bfloat16).float().item()
    assert np.array_equal(ref.bf16_rne(a), want)
    assert np.isnan(ref.bf16_rne(np.array([np.nan], dtype=np.float32)))[0]
    g = torch.Generator().manual_seed(0)
    r = torch.randn(4096, generator=g) * torch.logspace(-20, 20, 4096)
    assert np.array_equal(ref.bf16_rne(r.numpy()), r.to(torch.bfloat16).float().numpy())      # an independent RNE (torch's CPU cast)


def test_closed_forms_of_c_num_den():
    """One clip, Nt = 1 text row (ignored), Nv = 1, D = 8, every value chosen so the result is known by hand."""
    bf = lambda v: torch.tensor(v, dtype=torch.float32).to(torch.bfloat16).float().numpy()
    #            F             E           -> F - E (fp32)            -> c
    # col 0:   1.0           -2^-8            1 + 2^-8  (a tie)          1.0            (ties to even)
    # col 1:   1.0           -3 * 2^-8        1 + 3 * 2^-8 (a tie)       1 + 2^-6
    # col 2:   2.5            0.5             2.0                        2.0
    # col 3:   0.0            0.0             0.0                        0.0
    # col 4:  -4.0            4.0            -8.0                       -8.0
    # col 5:   256.0         -1.0             257.0 (a tie at ulp 2)     256.0
    # col 6:   3.0            1.0             2.0                        2.0
    # col 7:   0.5            0.25            0.25                       0.25
    F = bf([1.0, 1.0, 2.5, 0.0, -4.0, 256.0, 3.0, 0.5])
    E = bf([-2.0 ** -8, -3 * 2.0 ** -8, 0.5, 0.0, 4.0, -1.0, 1.0, 0.25])
    assert np.array_equal(E, np.array([-2.0 ** -8, -3 * 2.0 ** -8, 0.5, 0.0, 4.0, -1.0, 1.0, 0.25], dtype=np.float32))   # all bf16 values
    c_want = np.array([1.0, 1.0 + 2.0 ** -6, 2.0, 0.0, -8.0, 256.0, 2.0, 0.25], dtype=np.float32)
    p = bf([0.5, 1.0, 2.0, 0.0, 8.0, -256.0, 0.0, 0.25])
    x = np.concatenate([np.full((1, 1, 8), 77.0, dtype=np.float32), F.reshape(1, 1, 8)], axis=1)             # a text row in front
    f, c, sums = ref.probe_ref(x, E.reshape(1, 1, 8), p.reshape(1, 1, 8), Nt=1)
    assert np.array_equal(f.reshape(-1), F) and np.array_equal(c.reshape(-1), c_want)
    # |c - p| = 0.5, 2^-6, 0, 0, 16, 512, 2, 0 ; |p| = 0.5, 1, 2, 0, 8, 256, 0, 0.25
    assert sums[0, 0] == 0.5 + 2.0 ** -6 + 16 + 512 + 2 and sums[0, 1] == 0.5 + 1 + 2 + 8 + 256 + 0.25
    assert sc.distances(sums.tolist()) == [(530.5 + 2.0 ** -6) / 267.75]
    # a zero p: den = 0, the distance is inf and the step computes whatever the threshold
    _, _, z = ref.probe_ref(x, E.reshape(1, 1, 8), np.zeros((1, 1, 8), dtype=np.float32), Nt=1)
    assert z[0, 1] == 0.0 and z[0, 0] == float(np.abs(c_want).astype(np.float64).sum())
    assert sc.distances(z.tolist()) == [INF] and sc.decide(z.tolist(), INF)[0] is False
    # store and apply: t = bf16(X - F), rows = bf16(F + t); 1 + 2^-7 + 2^-7 ... X - F = 2^-8 + 1 - 1: pick a tie again
    X = x.copy()
    X[0, 1] = bf([1.0 + 2.0 ** -7, 3.0, 2.5, 1.0, -4.0, 257.0 + 1.0, 3.0, 0.75])     # 258 is a bf16 value
    t, p2 = ref.store_ref(X, f, c, Nt=1)
    assert np.array_equal(t.reshape(-1), np.array([2.0 ** -7, 2.0, 0.0, 1.0, 0.0, 2.0, 0.0, 0.25], dtype=np.float32)) and np.array_equal(p2, c)
    y = ref.apply_ref(x, t, Nt=1)
    assert np.array_equal(y[0, 0], x[0, 0])                                                                 # text row untouched
    assert np.array_equal(y[0, 1], np.array([1.0 + 2.0 ** -7, 3.0, 2.5, 1.0, -4.0, 258.0, 3.0, 0.75], dtype=np.float32))
    # and a rounding in apply: 256 + 1 = 257 is a tie at ulp 2 -> 256
    assert ref.apply_ref(np.full((1, 1, 1), 256.0, dtype=np.float32), np.ones((1, 1, 1), dtype=np.float32), Nt=0)[0, 0, 0] == 256.0


def test_decide_table():
    one = [(1.0, 4.0)]                       # d = 0.25
    assert sc.decide(one, 0.5) == (True, "threshold", 0.25, [0.25])
    assert sc.decide(one, 0.25) == (False, "threshold", 0.25, [0.25])            # strict: d < threshold
    assert sc.decide(one, 0.0)[0] is False
    assert sc.decide([(0.0, 4.0)], 0.0)[0] is False                              # threshold 0 never skips, not even an unchanged residual
    # one decision over all clips: the largest distance decides
    assert sc.decide([(1.0, 4.0), (3.0, 4.0)], 0.5) == (False, "threshold", 0.75, [0.25, 0.75])
    assert sc.decide([(1.0, 4.0), (3.0, 4.0)], 0.8)[0] is True
    # NaN computes, wherever it sits and whatever the threshold
    for sums in ([(NAN, 4.0)], [(1.0, NAN)], [(1.0, 4.0), (NAN, 4.0)], [(NAN, 0.0)]):
        skip, reason, dmax, d = sc.decide(sums, INF)
        assert skip is False and reason == "threshold" and math.isnan(dmax)
    # den == 0 computes (inf < inf is false)
    assert sc.decide([(1.0, 0.0)], INF)[:3] == (False, "threshold", INF)
    assert sc.decide([(0.0, 0.0)], INF)[:3] == (False, "threshold", INF)
    # the cap on consecutive skips
    assert sc.decide(one, INF, consecutive_skips=1, max_consecutive_skips=2)[:2] == (True, "threshold")
    assert sc.decide(one, INF, consecutive_skips=2, max_consecutive_skips=2)[:2] == (False, "cap")
    assert sc.decide(one, INF, consecutive_skips=0, max_consecutive_skips=0)[:2] == (False, "cap")
    assert sc.decide(one, INF, consecutive_skips=10 ** 6, max_consecutive_skips=None)[:2] == (True, "threshold")
    # forced wins over the cap and over the threshold; the distance is still reported
    assert sc.decide(one, INF, forced=True, consecutive_skips=2, max_consecutive_skips=2) == (False, "forced", 0.25, [0.25])
    # invalid state: nothing stored, or stored for another shape; no distance is reported
    assert sc.decide(None, INF, state="first", forced=True) == (False, "first", None, None)
    assert sc.decide(one, INF, state="shape") == (False, "shape", None, None)
    with pytest.raises(ValueError, match="supported"):
        sc.decide(one, INF, state="stale")
    assert set(sc.REASONS) == {"first", "forced", "cap", "shape", "threshold"}


def tiny_model(num_layers=2):
    from orv_amd.cogvideox_control import CogVideoXTransformer3DModelTraj
    return CogVideoXTransformer3DModelTraj(num_attention_heads=2, attention_head_dim=64, in_channels=8, out_channels=4, num_layers=num_layers,
                                           text_embed_dim=32, time_embed_dim=32, sample_width=12, sample_height=8, sample_frames=9,
                                           max_text_seq_length=8)


def test_python_surface_refusals_and_defaults():
    from orv_amd.cogvideox_control import CogVideoXImageToVideoPipelineTraj
    m = tiny_model()
    assert m._step_cache is None
    pipe = CogVideoXImageToVideoPipelineTraj(transformer=m, scheduler=None)
    assert pipe.transformer._step_cache is None and pipe.step_cache_report == []          # a fresh pipeline: the cache is off
    for bad in (-1e-9, NAN, "x", None):
        with pytest.raises(ValueError, match="supported: an inference forward"):
            m.enable_step_cache(bad)
        assert m._step_cache is None
    with pytest.raises(ValueError, match="max_consecutive_skips"):
        m.enable_step_cache(0.1, max_consecutive_skips=-1)
    with pytest.raises(ValueError, match="num_layers >= 2"):
        tiny_model(1).enable_step_cache(0.1)
    for kw in (dict(compute_first=0), dict(compute_last=-1), dict(compute_first=1.5)):
        with pytest.raises(ValueError, match="supported: an integer"):
            pipe.enable_step_cache(0.1, **kw)
    cache = pipe.enable_step_cache(0.25, max_consecutive_skips=3, compute_first=2, compute_last=0)
    assert cache is m._step_cache and cache.threshold == 0.25 and cache.max_consecutive_skips == 3 and cache.history == []
    assert cache.first_output is None and cache.first_residual is None and cache.tail_residual is None
    g0 = cache.generation
    cache.threshold = INF
    assert cache.threshold == INF
    with pytest.raises(ValueError):
        cache.threshold = -1.0
    assert pipe.enable_step_cache(0.5).generation == g0 + 1                               # a new generation: no stale graph replays
    assert pipe.disable_step_cache() is pipe and m._step_cache is None and pipe.step_cache_report == []


def test_c_abi_refusals():
    from orv_amd import _lib
    h = _lib.lib()
    err = lambda: h.orv_last_error().decode()
    buf = (ctypes.c_uint16 * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    q = ctypes.c_void_p(p.value + 1024)
    r = ctypes.c_void_p(p.value + 2048)
    s = ctypes.c_void_p(p.value + 3072)
    u = ctypes.c_void_p(p.value + 4096)
    assert h.orv_step_cache_scratch(1, 1, 64) == 2 and h.orv_step_cache_scratch(3, 1025, 64) == 3 * 2 * 9
    assert h.orv_step_cache_scratch(1, 1, 72) == -1 and "multiple of 64" in err()
    assert h.orv_step_cache_scratch(0, 1, 64) == -1 and "B = 0" in err()
    assert h.orv_step_cache_probe(p, q, r, s, None, p, 2, p, 1, 0, 1, 64, None) != 0 and "null pointer" in err()
    assert h.orv_step_cache_probe(p, q, r, s, u, p, 2, p, 1, 0, 1, 96, None) != 0 and "D = 96" in err()
    assert h.orv_step_cache_probe(p, q, r, s, u, p, 2, p, 1, -1, 1, 64, None) != 0 and "Nt = -1" in err()
    assert h.orv_step_cache_probe(p, q, r, s, u, p, 1, p, 1, 0, 1, 64, None) != 0 and "scratch holds 1 doubles" in err()
    assert h.orv_step_cache_probe(p, q, r, s, s, p, 2, p, 1, 0, 1, 64, None) != 0 and "must not alias" in err()
    assert h.orv_step_cache_probe(ctypes.c_void_p(p.value + 2), q, r, s, u, p, 2, p, 1, 0, 1, 64, None) != 0 and "16-byte aligned" in err()
    assert h.orv_step_cache_store(p, q, r, s, None, 1, 0, 1, 64, None) != 0 and "null pointer" in err()
    assert h.orv_step_cache_store(p, q, r, s, s, 1, 0, 1, 64, None) != 0 and "must not alias" in err()
    assert h.orv_step_cache_store(p, q, r, s, u, 70000, 0, 1, 64, None) != 0 and "B = 70000" in err()
    assert h.orv_step_cache_apply(p, None, 1, 0, 1, 64, None) != 0 and "null pointer" in err()
    assert h.orv_step_cache_apply(p, p, 1, 0, 1, 64, None) != 0 and "must not alias" in err()
    assert h.orv_step_cache_apply(p, q, 1, 0, 0, 64, None) != 0 and "Nv = 0" in err()


def test_header_and_ctypes_agree_on_the_step_cache_entries():
    from orv_amd import _lib
    header = open(os.path.join(ROOT, "include", "orv_mi355.h")).read()
    declared = {n for n in re.findall(r"\b(orv_[a-z0-9_]+)\s*\(", header) if n.startswith("orv_step_cache_")}
    assert declared == {"orv_step_cache_scratch", "orv_step_cache_probe", "orv_step_cache_store", "orv_step_cache_apply"}
    assert declared == {n for n in _lib.SIGNATURES if n.startswith("orv_step_cache_")}
    for n in declared:                        # one ctypes argument per declared parameter
        params = re.search(r"\b" + n + r"\s*\(([^;]*)\)\s*;", header).group(1)
        assert len(params.split(",")) == len(_lib.SIGNATURES[n][1]), n


def test_cache_refuses_a_forward_that_records_gradients_and_batch_chains(monkeypatch):
    """Both refusals come ahead of anything that touches the device, so CPU inputs reach them."""
    cfg, _, ins, w, _ = load_golden("fwd_actions")
    from orv_amd.cogvideox_control import CogVideoXTransformer3DModelTraj
    m = CogVideoXTransformer3DModelTraj(**cfg)
    m.load_state_dict(w)
    m.requires_grad_(True)
    call = lambda: m(ins["hidden_states"], ins["encoder_hidden_states"], {"actions": ins["actions"]}, ins["timestep"])
    m.enable_step_cache(0.1)
    with torch.enable_grad(), pytest.raises(RuntimeError, match="step cache: this forward records gradients; supported: an inference forward"):
        call()
    monkeypatch.setenv("ORV_CHAINS", "2")
    with torch.no_grad(), pytest.raises(RuntimeError, match="step cache: ORV_CHAINS = 2; supported: an inference forward"):
        call()
    monkeypatch.delenv("ORV_CHAINS")
    m.disable_step_cache()
    if not torch.cuda.is_available():
        with torch.no_grad(), pytest.raises(RuntimeError, match="MI355X only"):      # cache off: the forward's own first refusal again
            call()
