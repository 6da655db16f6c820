"""Developer measurement (not part of any test): the flat AdamW kernel alone in its three parameter-precision modes on the 2B model's flat
buffer (1.69 B elements), same box, interleaved round-robin, device events around every launch.

    python tools/adamw_precision_time.py [--elements N] [--rounds R] [--out FILE]

Bytes per element moved by the algorithm: p 2 + 2, g 2, m 4 + 4, v 4 + 4 = 22 (modes 0 and 2), + lo 2 + 2 = 26 (mode 1).  Prints, per mode,
the median / min / max time and the achieved bytes per second, and the ratio of mode 1 and mode 2 to the default; appends the same lines
to --out when given.  With ``--state-precision fp8`` the three modes of the fp8-moment kernel (``orv_adamw_flat_s8``: m and v one byte each plus
one scale byte per 256 elements, 10 + 2/256 bytes per element, + 4 for lo in mode 1) are measured in the same rounds beside the default kernel,
with their ratio to it.  Needs the GPU: there is no CPU path."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from orv_amd import ops  # noqa: E402

BYTES = {0: 22, 1: 26, 2: 22}
NAMES = {0: "bf16 (default)", 1: "split_fp32", 2: "stochastic"}
BYTES_S8 = {0: 10 + 2 / 256, 1: 14 + 2 / 256, 2: 10 + 2 / 256}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--elements", type=int, default=1_690_000_000)
    ap.add_argument("--segments", type=int, default=600)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--state-precision", default="fp32", choices=["fp32", "fp8"])
    ap.add_argument("--lagging-segments", action="store_true",
                    help="every segment's own step count one behind the global one (parameters that skipped a step): the fp8-moment kernel then "
                         "computes its bias corrections per segment on the device, as the other kernels always do")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "adamw_precision_time.py measures on the MI355X only"
    dev = torch.device("cuda:0")
    n = a.elements // 2048 * 2048
    per = n // 2048 // a.segments * 2048
    starts = [i * per for i in range(a.segments)] + [n]
    g = torch.Generator(device=dev).manual_seed(0)
    p = (torch.randn(n, device=dev, generator=g, dtype=torch.float32) * 0.02).to(torch.bfloat16)
    grad = (torch.randn(n, device=dev, generator=g, dtype=torch.float32) * 1e-3).to(torch.bfloat16)
    m = torch.zeros(n, device=dev)
    v = torch.zeros(n, device=dev)
    lo = torch.zeros(n, dtype=torch.int16, device=dev)
    seg_start = torch.tensor(starts, dtype=torch.int64, device=dev)
    active = torch.ones(a.segments, dtype=torch.uint8, device=dev)
    seg_step = torch.ones(a.segments, dtype=torch.int32, device=dev)
    clip = torch.ones(1, device=dev)
    fp8 = a.state_precision == "fp8"
    if fp8:
        m8, v8 = (torch.zeros(n, dtype=torch.uint8, device=dev) for _ in range(2))
        m_exp, v_exp = (torch.zeros(n // 256, dtype=torch.uint8, device=dev) for _ in range(2))
    legs = (0, "s8-0", "s8-1", "s8-2") if fp8 else (0, 1, 2)
    times = {k: [] for k in legs}
    step = 0
    for r in range(a.warmup + a.rounds):
        for mode in legs:
            step += 1
            seg_step.fill_(max(1, step - 1) if a.lagging_segments else step)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            if isinstance(mode, str):
                k = int(mode[-1])
                ops.adamw_flat_s8(p, grad, m8, v8, m_exp, v_exp, seg_start, active, 1e-5, 0.9, 0.95, 1e-8, 1e-3, step, clip, seg_step=seg_step,
                                  lo=lo if k == 1 else None, mode=k, seed=0)
            elif mode == 0:
                ops.adamw_flat(p, grad, m, v, seg_start, active, 1e-5, 0.9, 0.95, 1e-8, 1e-3, step, clip, seg_step=seg_step)
            else:
                ops.adamw_flat_ex(p, grad, m, v, seg_start, active, 1e-5, 0.9, 0.95, 1e-8, 1e-3, step, clip, seg_step=seg_step,
                                  lo=lo if mode == 1 else None, mode=mode, seed=0)
            e1.record()
            torch.cuda.synchronize()
            if r >= a.warmup:
                times[mode].append(e0.elapsed_time(e1))
    lines = [f"adamw_precision_time: {n} elements in {a.segments} segments, {a.rounds} interleaved rounds after {a.warmup} warm-up, "
             f"{torch.cuda.get_device_name(0)}" + (", segment step counts one behind the global count" if a.lagging_segments else "")]
    med = {k: statistics.median(t) for k, t in times.items()}
    if fp8:
        lines.append(f"  mode 0 {NAMES[0]:15s} fp32 moments median {med[0]:7.3f} ms  (min {min(times[0]):.3f}, max {max(times[0]):.3f})  "
                     f"{BYTES[0]} B/element  {BYTES[0] * n / med[0] / 1e9:.2f} TB/s")
        for k in (0, 1, 2):
            t = times[f"s8-{k}"]
            mk = med[f"s8-{k}"]
            lines.append(f"  mode {k} {NAMES[k]:15s} fp8 moments  median {mk:7.3f} ms  (min {min(t):.3f}, max {max(t):.3f})  "
                         f"{BYTES_S8[k]:.3f} B/element  {BYTES_S8[k] * n / mk / 1e9:.2f} TB/s  time x{mk / med[0]:.3f} of the default kernel "
                         f"({BYTES_S8[k] / BYTES[0]:.3f} from traffic alone)" + ("  SLOWER THAN THE DEFAULT KERNEL" if mk > med[0] else ""))
    else:
        for k in (0, 1, 2):
            lines.append(f"  mode {k} {NAMES[k]:15s} median {med[k]:7.3f} ms  (min {min(times[k]):.3f}, max {max(times[k]):.3f})  "
                         f"{BYTES[k]} B/element  {BYTES[k] * n / med[k] / 1e9:.2f} TB/s")
        bw = {k: BYTES[k] * n / med[k] for k in med}
        lines.append(f"  mode 1 / mode 0: time x{med[1] / med[0]:.3f} (26/22 = 1.182 from traffic alone), bytes per second x{bw[1] / bw[0]:.3f}"
                     + ("  BELOW 0.85 of the default kernel's rate" if bw[1] < 0.85 * bw[0] else ""))
        lines.append(f"  mode 2 / mode 0: time x{med[2] / med[0]:.3f} (1.000 if the hash hides under the memory time)")
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
