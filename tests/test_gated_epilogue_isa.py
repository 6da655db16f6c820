"""Drain guard for the row-operand epilogues of gemm_d8.hip (CPU, cross-compile only).  The vector-memory counter retires in order, so a load
issued behind a store can only be waited for with `s_waitcnt vmcnt(0)`, which also waits for that store's acknowledgement.  Up to round 6
the gated-residual epilogue (EPI 2) loaded its bias, gate values and residual rows behind the previous stores and used them at once: 41 full
drains in gemm_d8_kernel<192, 2> against 10 in the plain kernel, 27 against 7 at BN = 128, 68 against 13 at BN = 256.  Round 7 gathers bias
and gate before a tile's first store and rolls the residual rows one 64-column group ahead.  The cap asserted here, per kernel symbol:

    drains(EPI 2 or 3) <= drains(EPI 0) + BN / 64 + 1

Figures of this revision (EPI 0 / EPI 2 / EPI 3): gemm_d8_kernel<128> 7 / 8 / -, <192> 10 / 12 / 4, <256> 13 / 12 / 4; gemm_d8r192_kernel<128>
14 / 15 / -, <192> 20 / 16 / -.  A spill reload is itself a load behind a store, so an epilogue that spills cannot meet the cap: with 128
accumulator registers gemm_d8_kernel<256, 2> spilled (15 registers and 68 drains before round 7); it now reads the next tile's first W
fragments again behind the epilogue instead of keeping them across it, keeps output row numbers in 32 bits and has no second gate row."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
PAIRS = [("gemm_d8_kernel", 128), ("gemm_d8_kernel", 192), ("gemm_d8_kernel", 256), ("gemm_d8r192_kernel", 128), ("gemm_d8r192_kernel", 192)]


@pytest.fixture(scope="module")
def drains(tmp_path_factory):
    """{(kernel, BN, EPI): number of `s_waitcnt vmcnt(0)`} of every instantiation in gemm_d8.hip, compiled with the Makefile's flags."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    asm = tmp_path_factory.mktemp("d8") / "gemm_d8.s"
    src = os.path.join(ROOT, "orv_amd", "csrc", "gemm_d8.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value", "-w", "-S", "--cuda-device-only",
                        "-o", str(asm), src], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    out, cur = {}, None
    for line in open(asm):
        m = re.match(r"^_Z\S*?(gemm_d8\w*_kernel)ILi(\d+)ELi(\d+)E\S*:", line)
        if m:
            cur = (m.group(1), int(m.group(2)), int(m.group(3)))
            out[cur] = 0
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif cur and re.match(r"\s*s_waitcnt\b[^;]*vmcnt\(0\)", line):
            out[cur] += 1
    return out


@pytest.mark.parametrize("kernel,bn", PAIRS)
def test_row_operand_epilogues_drain_at_most_once_per_column_group(drains, kernel, bn):
    assert (kernel, bn, 0) in drains and (kernel, bn, 2) in drains, sorted(drains)
    cap = drains[(kernel, bn, 0)] + bn // 64 + 1
    for epi in (2, 3):
        if (kernel, bn, epi) in drains:
            print(f"{kernel}<{bn}, {epi}>: {drains[(kernel, bn, epi)]} drains, cap {cap} (plain kernel {drains[(kernel, bn, 0)]})")
            assert drains[(kernel, bn, epi)] <= cap, (kernel, bn, epi, drains[(kernel, bn, epi)], cap)
