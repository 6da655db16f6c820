"""numpy restatement of the two reductions behind FusedAdamW's parameter groups and skip guard (orv_amd/csrc/optim_groups.hip), in the
operation order that file states, so that the device results can be held to it bit for bit.

``segment_sumsq``  - per segment: 1024 lanes, lane t owns the runs x[8192 k + 8 t .. + 8) of the zero-padded segment and adds their squares
                     in ascending index into one fp64 accumulator (x^2 of a bf16 value is exact, so each step is one fp64 rounding), then
                     the lane sums are folded in halves (512, 256, ..., 1).
``step_guard``     - the global sum and one sum per group, each in ascending segment index from +0 (a segment is added or left out, never
                     multiplied by a mask); clip = fp32(c * inv_world), c = r if not r > 1 else 1, r = max_grad_norm / (sqrt(ss) * inv_world
                     + 1e-6) in fp64 (c = 1 when max_grad_norm == 0); with ``skip_nonfinite`` and a non-finite ss the mask is cleared, the
                     coefficient is 0, the running count goes up and the flag is 1."""
import numpy as np

LANES, RUN = 1024, 8
ROUND = LANES * RUN
MAX_GROUPS = 8
REPORT = 11          # ss, 8 group sums, running skip count, skipped


def segment_sumsq_one(x) -> np.float64:
    """x: the values of one segment (any float array holding bf16-representable values, padding included)."""
    x = np.asarray(x, dtype=np.float64).ravel()
    rounds = max(1, -(-x.size // ROUND))
    sq = np.zeros(rounds * ROUND, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        sq[:x.size] = x * x                                  # exact for bf16 values
        sq = sq.reshape(rounds, LANES, RUN)
        acc = np.zeros(LANES, dtype=np.float64)
        for k in range(rounds):
            for e in range(RUN):
                acc = acc + sq[k, :, e]
        o = LANES // 2
        while o > 0:
            acc[:o] = acc[:o] + acc[o:2 * o]
            o //= 2
    return acc[0]


def segment_sumsq(g, seg_start) -> np.ndarray:
    """g: the flat gradient values (float array), seg_start: nseg + 1 offsets -> fp64[nseg]."""
    g = np.asarray(g, dtype=np.float64)
    return np.array([segment_sumsq_one(g[int(a):int(b)]) for a, b in zip(seg_start[:-1], seg_start[1:])], dtype=np.float64)


def step_guard(seg_ss, seg_group, seg_active, max_grad_norm, inv_world=1.0, skip_nonfinite=False, skip_count=0.0):
    """-> (clip fp32, seg_active uint8 copy, report fp64[11]); ``skip_count``: report[9] before the call."""
    seg_ss = np.asarray(seg_ss, dtype=np.float64)
    sums = np.zeros(MAX_GROUPS + 1, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        for s, j in zip(seg_ss, seg_group):
            if int(j) < MAX_GROUPS:
                sums[int(j)] = sums[int(j)] + s
            sums[MAX_GROUPS] = sums[MAX_GROUPS] + s
        ss = sums[MAX_GROUPS]
        inv_world = np.float64(np.float32(inv_world))
        c = np.float64(1.0)
        if np.float32(max_grad_norm) != 0:
            r = np.float64(np.float32(max_grad_norm)) / (np.sqrt(ss) * inv_world + np.float64(1e-6))
            c = np.float64(1.0) if r > 1.0 else r
        skipped = bool(skip_nonfinite) and not np.isfinite(ss)
        clip = np.float32(0.0) if skipped else np.float32(c * inv_world)
    active = np.array(seg_active, dtype=np.uint8, copy=True)
    if skipped:
        active[:] = 0
    report = np.zeros(REPORT, dtype=np.float64)
    report[0] = ss
    report[1:1 + MAX_GROUPS] = sums[:MAX_GROUPS]
    report[9] = np.float64(skip_count) + (1.0 if skipped else 0.0)
    report[10] = 1.0 if skipped else 0.0
    return clip, active, report
