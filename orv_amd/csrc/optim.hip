// Opt-in parameter-precision modes of the flat fused AdamW (orv_adamw_flat_ex).  Mode 0 is the plain bf16 update
// of backward.hip (orv_adamw_flat_steps, untouched).  The two modes here run the same per-element formula in fp32
//      g *= clip ; m = b1 m + (1-b1) g ; v = b2 v + (1-b2) g^2 ; w = w (1 - lr wd) - lr (m / bc1) / (sqrt(v / bc2) + eps)
// (same clip, per-segment bias correction, decoupled decay, operation order and segment skip) and differ in what w is and how it is stored:
//
//   mode 1 "split_fp32": w is an exact fp32 master kept as the bf16 weight p plus a 16-bit low half lo:
//        master_bits = (p_bits << 16) + sign_extend(lo)                       (32-bit integer arithmetic)
//        p_bits = (master_bits + 0x8000) >> 16 ; lo = master_bits - (p_bits << 16)      (nearest, TIES AWAY from zero)
//      lo always lies in [-32768, 32767], so the round trip is exact for every finite master (nearest-even would leave lo = +-32768 on the
//      two kinds of exact tie, which 16 bits cannot tell apart).  A non-finite master writes the matching non-finite bf16 (NaN quiet), lo = 0.
//
//   mode 2 "stochastic": w is the bf16 weight; the fp32 result is stored as p_bits = (bits + r) >> 16 with r a uniform 16-bit integer,
//      so the expectation of the stored weight is the fp32 result.  r depends on (seed, step, flat element index i) ONLY:
//        mix(x): x ^= x >> 16 ; x *= 0x7feb352d ; x ^= x >> 15 ; x *= 0x846ca68b ; x ^= x >> 16         (all modulo 2^32)
//        key = mix(hi32(i) + mix(step + mix(seed)))
//        r(i) = mix(lo32(i) ^ key) >> 16
//      `step` is the `step` argument of the entry point (FusedAdamW.step_count), i the position in the flat buffer.  Launch geometry, wave,
//      time and rank do not enter: two runs are identical, a resumed run continues the sequence and all data-parallel ranks draw the same r.
//      Non-finite results are written unperturbed (NaN quiet); a finite result that r would carry into infinity becomes the largest finite bf16.
//
// Both modes share ONE device function for the fp32 arithmetic, compiled without FMA contraction, so that the fp32 result of mode 2 is
// bit for bit the mode-1 master of the same inputs with lo = 0 (tests/test_gpu_adamw_precision.py holds the rounding to that).
#include "common.hpp"

#pragma clang fp contract(off)

namespace {

struct AdamwCoef {
    float b1, b2, omb1, omb2, lr, eps, decay, ibc1, ibc2, clip;
};

// the fp32 arithmetic of every mode of this file: returns the new weight, updates the moments in place
__device__ __forceinline__ float adamw_fp32(float w, float g, float& m, float& v, const AdamwCoef& k) {
    const float gr = g * k.clip;
    m = k.b1 * m + k.omb1 * gr;
    v = k.b2 * v + k.omb2 * gr * gr;
    return w * k.decay - k.lr * (m * k.ibc1) / (sqrtf(v * k.ibc2) + k.eps);
}

__device__ __forceinline__ uint32_t mix32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

// MODE 1: split fp32 master (p + lo, 26 bytes of traffic per element); MODE 2: stochastic rounding (22 bytes).
// A workgroup owns 2048 consecutive elements = part of one segment, 8 per lane, 16-byte accesses (lo: one 16-byte access per lane).
// GROUPS: lr and wd are those of the segment's parameter group (orv_adamw_flat_groups), picked once per workgroup - a workgroup never
// straddles a segment - from the by-value table with scalar selects (no indexed access, so the table never leaves the kernel arguments).
template <int MODE, bool GROUPS>
__device__ __forceinline__ void adamw_flat_ex_body(bf16_t* __restrict__ p, int16_t* __restrict__ lo16, const bf16_t* __restrict__ g,
                                                   float* __restrict__ m, float* __restrict__ v, const long* __restrict__ seg_start,
                                                   const uint8_t* __restrict__ active, int nseg, float lr, float b1, float b2, float eps,
                                                   float wd, float bc1, float bc2, const float* __restrict__ clip,
                                                   const int* __restrict__ seg_step, uint32_t seed, uint32_t step,
                                                   const uint8_t* __restrict__ seg_group, const orv_adamw_groups_t& groups) {
    const long e0 = (long)blockIdx.x * 2048;
    int lo = 0, hi = nseg - 1;                 // last segment with seg_start <= e0 (wave-uniform binary search)
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (seg_start[mid] <= e0) lo = mid; else hi = mid - 1; }
    // the group byte decides the branch together with the activity byte (a group outside the table: the segment is left alone), so the
    // two loads are in flight together instead of one behind the other
    const int gi = GROUPS ? seg_group[lo] : 0;
    if (!active[lo] | (gi >= ORV_ADAMW_MAX_GROUPS)) return;
    if (GROUPS) {
#pragma unroll
        for (int j = 0; j < ORV_ADAMW_MAX_GROUPS; ++j)
            if (gi == j) { lr = groups.lr[j]; wd = groups.weight_decay[j]; }
    }
    if (seg_step) {                            // one step count PER PARAMETER (bias correction), as in adamw_flat_kernel
        const float st = (float)seg_step[lo];
        bc1 = 1.f - powf(b1, st);
        bc2 = 1.f - powf(b2, st);
    }
    AdamwCoef k;
    k.b1 = b1; k.b2 = b2; k.omb1 = 1.f - b1; k.omb2 = 1.f - b2; k.lr = lr; k.eps = eps;
    k.decay = 1.f - lr * wd; k.ibc1 = 1.f / bc1; k.ibc2 = 1.f / bc2; k.clip = clip ? *clip : 1.f;
    const long i = e0 + threadIdx.x * 8;
    const uint4 up = *(const uint4*)(p + i), ug = *(const uint4*)(g + i);
    float4 m0 = *(const float4*)(m + i), m1 = *(const float4*)(m + i + 4), v0 = *(const float4*)(v + i), v1 = *(const float4*)(v + i + 4);
    float mm[8] = {m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, m1.z, m1.w}, vv[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
    const uint32_t wp[4] = {up.x, up.y, up.z, up.w}, wg[4] = {ug.x, ug.y, ug.z, ug.w};
    uint32_t wl[4] = {0u, 0u, 0u, 0u};
    if (MODE == 1) { const uint4 ul = *(const uint4*)(lo16 + i); wl[0] = ul.x; wl[1] = ul.y; wl[2] = ul.z; wl[3] = ul.w; }
    const uint32_t key = MODE == 2 ? mix32((uint32_t)((unsigned long)i >> 32) + mix32(step + mix32(seed))) : 0u;
    uint32_t np[8], nl[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const uint32_t pb = (e & 1) ? wp[e >> 1] >> 16 : wp[e >> 1] & 0xffffu;
        const uint32_t gb = (e & 1) ? wg[e >> 1] >> 16 : wg[e >> 1] & 0xffffu;
        uint32_t wbits = pb << 16;
        if (MODE == 1) wbits += (uint32_t)(int32_t)(int16_t)((e & 1) ? wl[e >> 1] >> 16 : wl[e >> 1] & 0xffffu);
        const uint32_t u = __float_as_uint(adamw_fp32(__uint_as_float(wbits), bf2f((bf16_t)gb), mm[e], vv[e], k));
        const uint32_t a = u & 0x7fffffffu;
        if (a >= 0x7f800000u) {                // infinity / NaN: the matching bf16 (NaN kept quiet), no low half, no perturbation
            np[e] = (u >> 16) | (a > 0x7f800000u ? 0x40u : 0u);
            nl[e] = 0u;
        } else if (MODE == 1) {
            np[e] = (u + 0x8000u) >> 16;
            nl[e] = (u - (np[e] << 16)) & 0xffffu;
        } else {
            const uint32_t t = u + (mix32((uint32_t)(i + e) ^ key) >> 16);
            np[e] = (t & 0x7fffffffu) >= 0x7f800000u ? ((u >> 16) & 0x8000u) | 0x7f7fu : t >> 16;
            nl[e] = 0u;
        }
    }
    *(float4*)(m + i) = make_float4(mm[0], mm[1], mm[2], mm[3]); *(float4*)(m + i + 4) = make_float4(mm[4], mm[5], mm[6], mm[7]);
    *(float4*)(v + i) = make_float4(vv[0], vv[1], vv[2], vv[3]); *(float4*)(v + i + 4) = make_float4(vv[4], vv[5], vv[6], vv[7]);
    *(uint4*)(p + i) = make_uint4(np[0] | np[1] << 16, np[2] | np[3] << 16, np[4] | np[5] << 16, np[6] | np[7] << 16);
    if (MODE == 1)
        *(uint4*)(lo16 + i) = make_uint4(nl[0] | nl[1] << 16, nl[2] | nl[3] << 16, nl[4] | nl[5] << 16, nl[6] | nl[7] << 16);
}

template <int MODE>
__global__ __launch_bounds__(256) void adamw_flat_ex_kernel(bf16_t* __restrict__ p, int16_t* __restrict__ lo16,
                                                            const bf16_t* __restrict__ g, float* __restrict__ m,
                                                            float* __restrict__ v, const long* __restrict__ seg_start,
                                                            const uint8_t* __restrict__ active, int nseg, float lr, float b1,
                                                            float b2, float eps, float wd, float bc1, float bc2,
                                                            const float* __restrict__ clip, const int* __restrict__ seg_step,
                                                            uint32_t seed, uint32_t step) {
    adamw_flat_ex_body<MODE, false>(p, lo16, g, m, v, seg_start, active, nseg, lr, b1, b2, eps, wd, bc1, bc2, clip, seg_step, seed, step,
                                    nullptr, orv_adamw_groups_t{});
}

// the same body; lr and weight decay per parameter group
template <int MODE>
__global__ __launch_bounds__(256) void adamw_flat_groups_kernel(bf16_t* __restrict__ p, int16_t* __restrict__ lo16,
                                                                const bf16_t* __restrict__ g, float* __restrict__ m,
                                                                float* __restrict__ v, const long* __restrict__ seg_start,
                                                                const uint8_t* __restrict__ active, int nseg, float b1, float b2,
                                                                float eps, float bc1, float bc2, const float* __restrict__ clip,
                                                                const int* __restrict__ seg_step, uint32_t seed, uint32_t step,
                                                                const uint8_t* __restrict__ seg_group, const orv_adamw_groups_t groups) {
    adamw_flat_ex_body<MODE, true>(p, lo16, g, m, v, seg_start, active, nseg, 0.f, b1, b2, eps, 0.f, bc1, bc2, clip, seg_step, seed, step,
                                   seg_group, groups);
}

}  // namespace

extern "C" int orv_adamw_flat_ex(void* p, const void* g, float* m, float* v, long n, const long* seg_start,
                                 const unsigned char* seg_active, const int* seg_step, int nseg, float lr, float beta1,
                                 float beta2, float eps, float weight_decay, int step, const float* clip_coef, void* lo, int mode,
                                 unsigned seed, void* stream) {
    ORV_REQUIRE(mode >= 0 && mode <= 2, "orv_adamw_flat_ex: mode=%d (0 bf16, 1 split_fp32, 2 stochastic)", mode);
    if (mode == 0)                             // the plain bf16 update: the existing kernel, lo ignored
        return orv_adamw_flat_steps(p, g, m, v, n, seg_start, seg_active, seg_step, nseg, lr, beta1, beta2, eps, weight_decay, step,
                                    clip_coef, stream);
    ORV_REQUIRE(p && g && m && v && seg_start && seg_active && nseg > 0 && step > 0, "orv_adamw_flat_ex: bad arguments");
    ORV_REQUIRE(n > 0 && n % 2048 == 0, "orv_adamw_flat_ex: n=%ld must be a multiple of 2048 (pad every segment)", n);
    ORV_REQUIRE(mode != 1 || lo, "orv_adamw_flat_ex: mode 1 (split_fp32) needs the low-half buffer lo (int16[n])");
    const float bc1 = 1.f - powf(beta1, (float)step), bc2 = 1.f - powf(beta2, (float)step);
    const dim3 grid((unsigned)(n / 2048)), block(256);
    if (mode == 1)
        hipLaunchKernelGGL(adamw_flat_ex_kernel<1>, grid, block, 0, (hipStream_t)stream, (bf16_t*)p, (int16_t*)lo, (const bf16_t*)g, m, v,
                           seg_start, seg_active, nseg, lr, beta1, beta2, eps, weight_decay, bc1, bc2, clip_coef, seg_step, seed,
                           (uint32_t)step);
    else
        hipLaunchKernelGGL(adamw_flat_ex_kernel<2>, grid, block, 0, (hipStream_t)stream, (bf16_t*)p, (int16_t*)nullptr, (const bf16_t*)g, m,
                           v, seg_start, seg_active, nseg, lr, beta1, beta2, eps, weight_decay, bc1, bc2, clip_coef, seg_step, seed,
                           (uint32_t)step);
    return orv_check_launch("orv_adamw_flat_ex");
}

extern "C" int orv_adamw_flat_groups(void* p, const void* g, float* m, float* v, long n, const long* seg_start,
                                     const unsigned char* seg_active, const int* seg_step, int nseg, const unsigned char* seg_group,
                                     orv_adamw_groups_t groups, float beta1, float beta2, float eps, int step, const float* clip_coef,
                                     void* lo, int mode, unsigned seed, void* stream) {
    ORV_REQUIRE(mode >= 0 && mode <= 2, "orv_adamw_flat_groups: mode=%d (0 bf16, 1 split_fp32, 2 stochastic)", mode);
    ORV_REQUIRE(groups.ngroups >= 1 && groups.ngroups <= ORV_ADAMW_MAX_GROUPS, "orv_adamw_flat_groups: ngroups=%d (supported: 1..%d)",
                groups.ngroups, ORV_ADAMW_MAX_GROUPS);
    ORV_REQUIRE(seg_group, "orv_adamw_flat_groups: null seg_group (one group index per segment, on the device)");
    if (mode == 0)                             // the plain bf16 update lives beside its parent kernel (backward.hip)
        return orv_adamw_flat_groups_bf16(p, g, m, v, n, seg_start, seg_active, seg_step, nseg, seg_group, groups, beta1, beta2, eps, step,
                                           clip_coef, stream);
    ORV_REQUIRE(p && g && m && v && seg_start && seg_active && nseg > 0 && step > 0, "orv_adamw_flat_groups: bad arguments");
    ORV_REQUIRE(n > 0 && n % 2048 == 0, "orv_adamw_flat_groups: n=%ld must be a multiple of 2048 (pad every segment)", n);
    ORV_REQUIRE(mode != 1 || lo, "orv_adamw_flat_groups: mode 1 (split_fp32) needs the low-half buffer lo (int16[n])");
    const float bc1 = 1.f - powf(beta1, (float)step), bc2 = 1.f - powf(beta2, (float)step);
    const dim3 grid((unsigned)(n / 2048)), block(256);
    if (mode == 1)
        hipLaunchKernelGGL(adamw_flat_groups_kernel<1>, grid, block, 0, (hipStream_t)stream, (bf16_t*)p, (int16_t*)lo, (const bf16_t*)g, m,
                           v, seg_start, seg_active, nseg, beta1, beta2, eps, bc1, bc2, clip_coef, seg_step, seed, (uint32_t)step,
                           seg_group, groups);
    else
        hipLaunchKernelGGL(adamw_flat_groups_kernel<2>, grid, block, 0, (hipStream_t)stream, (bf16_t*)p, (int16_t*)nullptr,
                           (const bf16_t*)g, m, v, seg_start, seg_active, nseg, beta1, beta2, eps, bc1, bc2, clip_coef, seg_step, seed,
                           (uint32_t)step, seg_group, groups);
    return orv_check_launch("orv_adamw_flat_groups");
}
