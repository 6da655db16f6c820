"""Host logic of the forward-attention dispatch (no GPU work): which kernel each entry point launches, through `ops.attention_kernel_name`
(the pick function the launches themselves use, attention.hip `attn_pick`).  The expectations are the selection the five entry points have
always made, written out; a change that sends the headline shape - or any row below - to another kernel should be a decision, not an accident.
The process switches are read once per process, so every switch gets a fresh child."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from orv_amd import ops  # noqa: E402

B, S, H = 4, 3226, 30                   # the headline shape
FUSED, PLAIN = 0.6931471805599453, 0.125    # scale * log2(e) == 1 (q pre-multiplied) / the plain 1 / sqrt(64)
BOUND = 11.8                            # random-init qk-LayerNorm
FWD, FWD_VT, BOUNDED, PACKED, DEV = 0, 1, 2, 3, 4

PP, PP_STATIC = "attn_fwd_pp_kernel<false>", "attn_fwd_pp_kernel<true>"
V2, V2_PLAIN, V2_STATIC = "attn_fwd_v2_kernel<true, true>", "attn_fwd_v2_kernel<true, false>", "attn_fwd_v2_kernel<true, true, true>"
V1, V1_PLAIN = "attn_fwd_v1_kernel<true, true>", "attn_fwd_v1_kernel<true, false>"
M16, W64 = "attn_fwd_m16_kernel", "attn_fwd_w64_kernel"
PAIR = "attn_fwd_pp_kernel<true> + attn_fwd_pp_kernel<false>"

# row -> (entry point, scale, score_bound, aligned_out)
ROWS = {
    "fwd aligned": (FWD, FUSED, 0.0, True),
    "fwd unaligned": (FWD, FUSED, 0.0, False),
    "fwd plain scale": (FWD, PLAIN, 0.0, True),
    "fwd vT": (FWD_VT, FUSED, 0.0, True),
    "fwd vT plain scale": (FWD_VT, PLAIN, 0.0, True),
    "bounded aligned": (BOUNDED, FUSED, BOUND, True),
    "bounded unaligned": (BOUNDED, FUSED, BOUND, False),
    "bounded aligned 61": (BOUNDED, FUSED, 61.0, True),
    "bounded unaligned 61": (BOUNDED, FUSED, 61.0, False),
    "bounded aligned 91": (BOUNDED, FUSED, 91.0, True),
    "bounded plain scale": (BOUNDED, PLAIN, BOUND, True),
    "bounded no bound": (BOUNDED, FUSED, 0.0, True),
    "packed": (PACKED, FUSED, BOUND, True),
    "dev aligned": (DEV, FUSED, 0.0, True),
    "dev unaligned": (DEV, FUSED, 0.0, False),
    "dev plain scale": (DEV, PLAIN, 0.0, True),
}

DEFAULT = {
    "fwd aligned": PP,
    "fwd unaligned": V2,
    "fwd plain scale": V2_PLAIN,
    "fwd vT": V1,
    "fwd vT plain scale": V1_PLAIN,
    "bounded aligned": PP_STATIC,               # the headline launch
    "bounded unaligned": V2_STATIC,
    "bounded aligned 61": PP_STATIC,            # limit 90 for the shift-free ping-pong kernel
    "bounded unaligned 61": V2,                 # limit 60 for the v2 kernel that shifts by the bound: online softmax
    "bounded aligned 91": PP,
    "bounded plain scale": V2_PLAIN,
    "bounded no bound": PP,
    "packed": PP_STATIC,
    "dev aligned": PAIR,
    "dev unaligned": V2,
    "dev plain scale": V2_PLAIN,
}

# every row a switch changes; the packed entry point looks at ORV_ATTN_W64 and ORV_ATTN_M16 only
SWITCHED = {
    "ORV_ATTN_PP=0": {"fwd aligned": V2, "bounded aligned": V2_STATIC, "bounded aligned 61": V2, "bounded aligned 91": V2,
                      "bounded no bound": V2, "dev aligned": V2},
    "ORV_ATTN_STATIC=0": {"bounded aligned": PP, "bounded unaligned": V2, "bounded aligned 61": PP, "dev aligned": PP},
    "ORV_ATTN_M16=1": {"bounded aligned": M16, "bounded aligned 61": M16, "packed": M16},
    "ORV_ATTN_W64=1": {"bounded aligned": W64, "bounded aligned 61": W64, "packed": W64},
}


def _names():
    return {row: ops.attention_kernel_name(entry, B, S, H, scale, bound, aligned) for row, (entry, scale, bound, aligned) in ROWS.items()}


def _clean_env():
    return {k: v for k, v in os.environ.items() if not k.startswith("ORV_ATTN_")}


def test_default_selection_at_the_headline_shape():
    assert not any(k.startswith("ORV_ATTN_") for k in os.environ), "run the suite without ORV_ATTN_* switches"
    assert set(DEFAULT) == set(ROWS)
    assert _names() == DEFAULT


def test_selection_does_not_depend_on_the_shape():
    for b, s, h in ((1, 80, 2), (2, 256, 30), (1, 257, 1)):
        got = {row: ops.attention_kernel_name(entry, b, s, h, scale, bound, aligned) for row, (entry, scale, bound, aligned) in ROWS.items()}
        assert got == DEFAULT, (b, s, h)


def test_each_switch_in_a_child_process():
    for switch, changed in SWITCHED.items():
        assert set(changed) <= set(ROWS) and all(DEFAULT[row] != name for row, name in changed.items()), switch
        name, value = switch.split("=")
        r = subprocess.run([sys.executable, os.path.abspath(__file__)], cwd=ROOT, env=dict(_clean_env(), **{name: value}), capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, (switch, r.stdout[-2000:], r.stderr[-2000:])
        got = dict(line[len("ROW "):].split(" -> ") for line in r.stdout.splitlines() if line.startswith("ROW "))
        assert got == dict(DEFAULT, **changed), switch


def test_the_packed_entry_point_refuses_what_its_launch_refuses():
    import pytest
    for scale, bound in ((PLAIN, BOUND), (FUSED, 0.0), (FUSED, 91.0)):
        with pytest.raises(RuntimeError, match="orv_attention_kernel_name"):
            ops.attention_kernel_name(PACKED, B, S, H, scale, bound, True)


if __name__ == "__main__":             # the child of test_each_switch_in_a_child_process
    for row_, name_ in _names().items():
        print(f"ROW {row_} -> {name_}")
