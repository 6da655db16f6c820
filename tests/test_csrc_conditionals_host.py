"""The kernel sources carry no build-time variants (CPU, reads source text only).  Probe, ablation, trace and alternative-schedule builds used
to live in orv_amd/csrc as preprocessor branches the shipped build never took; they were removed (README.md, "Build-time macros").  What may still
be conditional on an ORV_ macro is an overridable CONSTANT - a value, not alternative code."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "orv_amd", "csrc")
ALLOWED = re.compile(r"ORV_(D8_RATE_\w+|D8R192_RATE_\w+|T8R192_RATE_\w+|D8_CBP256|D8_CBP192|LN_WAVES|LNR_WAVES|ATTN_M16_DEFAULT|ATTN_W64_DEFAULT)")
CONDITIONAL = re.compile(r"^\s*#\s*(if|ifdef|ifndef|elif)\b(.*)$")


def _sources():
    names = sorted(n for n in os.listdir(CSRC) if os.path.isfile(os.path.join(CSRC, n)))
    assert len(names) >= 20, names
    return [(n, open(os.path.join(CSRC, n), errors="replace").read()) for n in names]


def test_preprocessor_conditionals_name_overridable_constants_only():
    seen, bad = 0, []
    for name, text in _sources():
        for no, line in enumerate(text.splitlines(), 1):
            m = CONDITIONAL.match(line)
            if not m:
                continue
            expr = m.group(2).split("//")[0]
            for macro in re.findall(r"\bORV_\w+", expr):
                seen += 1
                if not ALLOWED.fullmatch(macro):
                    bad.append("%s:%d: %s" % (name, no, macro))
    assert not bad, "build-time variant in the kernel sources:\n" + "\n".join(bad)
    assert seen >= 9, seen      # the scan sees the overridable constants (a regex that matches nothing would pass the assertion above)


def test_four_wave_gemm_experiment_is_gone():
    for name, text in _sources():
        for token in ("gemm_t4_kernel", "launch_t4"):
            assert token not in text, (name, token)
