// The two device-side reductions behind FusedAdamW's parameter groups, per-parameter gradient norms and skip guard (orv_segment_sumsq,
// orv_step_guard).  The per-group update kernels live beside their parents (backward.hip, optim.hip, optim_s8.hip), whose
// device functions they share.  Both reductions are in fp64, without atomics, in an order that this comment fixes, so that a host
// restatement (tests/adamw_groups_ref.py) follows them bit for bit.
//
// orv_segment_sumsq - out[s] = sum of g^2 over segment s = the L = seg_start[s + 1] - seg_start[s] bf16 elements from seg_start[s].
//   One workgroup of 1024 lanes per segment, one launch for the whole table.  THE ORDER, for a segment x[0 .. L):
//     1. Think of x padded with zeros to a multiple of 8192 and cut into rounds k = 0, 1, ... of 8192 elements, a round into 1024 runs of
//        8: lane t owns the runs x[8192 k + 8 t .. + 8).
//     2. Lane t starts at acc_t = +0 and adds, round after round and inside a run in ascending index, acc_t = acc_t + x^2.  x^2 is exact
//        (a bf16 has 8 significant bits), so every step is ONE fp64 rounding (the kernel issues it as fma(x, x, acc_t), the same value).
//        The padding adds nothing: acc_t + 0 = acc_t, and the kernel simply does not read it.
//     3. The 1024 lane sums are folded in halves: for o = 512, 256, ... , 1: acc_t = acc_t + acc_{t + o} for t < o.  out[s] = acc_0.
//   Only L enters: not the grid, not the other segments, not time.  A NaN or an infinity in x makes out[s] non-finite and touches no other
//   segment's sum.  L = 0 gives +0.
//
// orv_step_guard - one workgroup; lanes 0 .. 7 each add the sums of one group, lane 8 adds all of them, every one in ascending segment
//   index from +0 (a lane adds seg_ss[i] or skips it - it never multiplies by a mask, so a non-finite segment reaches its own group's sum
//   and the global one only).  Then, in fp64:
//        norm = sqrt(ss) * inv_world ; r = max_grad_norm / (norm + 1e-6) ; c = 1 if r > 1 else r     (so a NaN r stays; c = 1 when
//        max_grad_norm == 0) ; clip = fp32(c * inv_world)
//   and, when skip_nonfinite is set and ss is not finite: every byte of seg_active is cleared, clip = 0, the running count report[9] goes
//   up by one and report[10] = 1 (else 0).  report[0] = ss, report[1 + j] = the sum of group j (+0 for a group without segments).
#include "common.hpp"

#pragma clang fp contract(off)

namespace {

constexpr int kSsLanes = 1024;                 // lanes per segment
constexpr long kSsRound = (long)kSsLanes * 8;  // elements per round

__device__ __forceinline__ double ss_add8(double acc, const uint4 u) {
    const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const double a = (double)bf2f((bf16_t)(w[e] & 0xffffu)), b = (double)bf2f((bf16_t)(w[e] >> 16));
        acc = __builtin_fma(a, a, acc);
        acc = __builtin_fma(b, b, acc);
    }
    return acc;
}

__global__ __launch_bounds__(kSsLanes) void segment_sumsq_kernel(const bf16_t* __restrict__ g, const long* __restrict__ seg_start,
                                                                 double* __restrict__ out) {
    __shared__ double red[kSsLanes];
    const int t = threadIdx.x;
    const long a = seg_start[blockIdx.x], L = seg_start[blockIdx.x + 1] - a;
    const bf16_t* x = g + a;
    double acc = 0.0;
    long i = (long)t * 8;
    // eight rounds' loads in flight per lane (one workgroup streams a whole segment: 128 KB in flight); the additions keep the order
    // of the rounds
    for (; i + 7 * kSsRound + 8 <= L; i += 8 * kSsRound) {
        uint4 u[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) u[k] = *(const uint4*)(x + i + k * kSsRound);
#pragma unroll
        for (int k = 0; k < 8; ++k) acc = ss_add8(acc, u[k]);
    }
    for (; i + 8 <= L; i += kSsRound) acc = ss_add8(acc, *(const uint4*)(x + i));
    for (long j = i; j < L; ++j) {             // the one run that L cuts short (L % 8 != 0)
        const double v = (double)bf2f(x[j]);
        acc = __builtin_fma(v, v, acc);
    }
    red[t] = acc;
    __syncthreads();
    for (int o = kSsLanes / 2; o > 0; o >>= 1) {
        if (t < o) red[t] = red[t] + red[t + o];
        __syncthreads();
    }
    if (t == 0) out[blockIdx.x] = red[0];
}

constexpr int kGuardTile = 2048;               // segment sums staged in LDS per pass

__global__ __launch_bounds__(256) void step_guard_kernel(const double* __restrict__ seg_ss, const uint8_t* __restrict__ seg_group, int nseg,
                                                         float max_grad_norm, float inv_world, int skip_nonfinite,
                                                         uint8_t* __restrict__ seg_active, float* __restrict__ clip_coef,
                                                         double* __restrict__ report) {
    __shared__ double tile[kGuardTile];
    __shared__ uint8_t grp[kGuardTile];
    __shared__ double sums[ORV_ADAMW_MAX_GROUPS + 1];
    const int t = threadIdx.x;
    double acc = 0.0;                          // lane j < 8: group j; lane 8: every segment
    for (int base = 0; base < nseg; base += kGuardTile) {
        const int cnt = min(kGuardTile, nseg - base);
        for (int i = t; i < cnt; i += 256) { tile[i] = seg_ss[base + i]; grp[i] = seg_group[base + i]; }
        __syncthreads();
        if (t <= ORV_ADAMW_MAX_GROUPS)
            for (int i = 0; i < cnt; ++i)
                if (t == ORV_ADAMW_MAX_GROUPS || grp[i] == t) acc = acc + tile[i];
        __syncthreads();
    }
    if (t <= ORV_ADAMW_MAX_GROUPS) sums[t] = acc;
    __syncthreads();
    const double ss = sums[ORV_ADAMW_MAX_GROUPS];
    const bool skipped = skip_nonfinite && !__builtin_isfinite(ss);
    if (skipped)
        for (int i = t; i < nseg; i += 256) seg_active[i] = 0;
    if (t == 0) {
        double c = 1.0;
        if (max_grad_norm != 0.f) {
            const double r = (double)max_grad_norm / (sqrt(ss) * (double)inv_world + 1e-6);
            c = r > 1.0 ? 1.0 : r;
        }
        *clip_coef = skipped ? 0.f : (float)(c * (double)inv_world);
        report[0] = ss;
        for (int j = 0; j < ORV_ADAMW_MAX_GROUPS; ++j) report[1 + j] = sums[j];
        report[9] = report[9] + (skipped ? 1.0 : 0.0);
        report[10] = skipped ? 1.0 : 0.0;
    }
}

}  // namespace

extern "C" int orv_segment_sumsq(const void* g, const long* seg_start, int nseg, double* out, void* stream) {
    ORV_REQUIRE(g && seg_start && out, "orv_segment_sumsq: null buffer (g bf16, seg_start int64[nseg + 1], out fp64[nseg], all on the device)");
    ORV_REQUIRE(nseg > 0, "orv_segment_sumsq: nseg=%d must be positive", nseg);
    ORV_REQUIRE(orv_aligned(g, 16), "orv_segment_sumsq: g must be 16-byte aligned");
    hipLaunchKernelGGL(segment_sumsq_kernel, dim3((unsigned)nseg), dim3(kSsLanes), 0, (hipStream_t)stream, (const bf16_t*)g, seg_start, out);
    return orv_check_launch("orv_segment_sumsq");
}

extern "C" int orv_step_guard(const double* seg_ss, const unsigned char* seg_group, int nseg, float max_grad_norm, float inv_world,
                              int skip_nonfinite, unsigned char* seg_active, float* clip_coef, double* report, void* stream) {
    ORV_REQUIRE(seg_ss && seg_group && seg_active && clip_coef && report,
                "orv_step_guard: null buffer (seg_ss fp64[nseg], seg_group / seg_active bytes[nseg], clip_coef fp32[1], report fp64[%d])",
                ORV_GUARD_REPORT);
    ORV_REQUIRE(nseg > 0, "orv_step_guard: nseg=%d must be positive", nseg);
    ORV_REQUIRE(max_grad_norm >= 0.f && inv_world > 0.f && inv_world <= 1.f,
                "orv_step_guard: max_grad_norm=%g must not be negative (0: no clipping) and inv_world=%g must lie in (0, 1]",
                (double)max_grad_norm, (double)inv_world);
    hipLaunchKernelGGL(step_guard_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, seg_ss, seg_group, nseg, max_grad_norm, inv_world,
                       skip_nonfinite, seg_active, clip_coef, report);
    return orv_check_launch("orv_step_guard");
}
