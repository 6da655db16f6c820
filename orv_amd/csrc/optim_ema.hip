// Exponential moving average of the weights on the flat buffers of the fused optimizers (orv_amd.FusedEMA).
//
// The shadow s is ONE fp32 buffer in the segment layout of the optimizer's flat parameter buffer p (bf16[n], every segment padded to 2048
// elements, padding zero).  theta is the weight the average follows:
//      the fp32 master (p_bits << 16) + sign_extend(lo)     where the optimizer keeps low halves lo (int16[n], orv_adamw_flat_ex mode 1),
//      fp32(p), exactly                                      otherwise.
//
//   orv_ema_update:   s <- s - omd * (s - theta)             omd = fp32(1 - decay), computed on the host
//      Three fp32 operations per element in exactly this order, each rounded on its own (no FMA contraction), so that a numpy restatement
//      (tests/ema_ref.py) gives the same bits.  Padding: s = theta = +0 gives 0 - omd * 0 = +0 for every finite omd - no segment table needed.
//      Traffic: 4 (s read) + 4 (s write) + 2 (p) bytes per element, + 2 (lo) with masters.
//
//   orv_ema_swap_in:  stash_p <- p ; stash_lo <- lo ; p <- bf16_rne(s)              (stash_* may be NULL: nothing is kept)
//                     zero_lo != 0: lo <- 0, so that the master equals the written bf16 value
//      bf16_rne is round-to-nearest-even on the bit pattern (u + 0x7fff + ((u >> 16) & 1)) >> 16; a NaN keeps its sign and upper payload
//      with the quiet bit set.  Traffic: 4 (s) + 2 (p read) + 2 (stash_p) + 2 (p write), + 2 (lo read) + 2 (stash_lo) with masters.
//
// Geometry of the AdamW kernels: a workgroup owns 2048 consecutive elements, 8 per lane, 16-byte accesses.  No atomics, no LDS, no
// cross-lane traffic: every element depends on its own inputs only, so the result is independent of launch geometry, time and rank.
#include "common.hpp"

#pragma clang fp contract(off)

namespace {

template <bool MASTER>
__global__ __launch_bounds__(256) void ema_update_kernel(float* __restrict__ s, const bf16_t* __restrict__ p,
                                                         const int16_t* __restrict__ lo16, float omd) {
    const long i = (long)blockIdx.x * 2048 + threadIdx.x * 8;
    const uint4 up = *(const uint4*)(p + i);
    const float4 s0 = *(const float4*)(s + i), s1 = *(const float4*)(s + i + 4);
    uint32_t wl[4] = {0u, 0u, 0u, 0u};
    if (MASTER) { const uint4 ul = *(const uint4*)(lo16 + i); wl[0] = ul.x; wl[1] = ul.y; wl[2] = ul.z; wl[3] = ul.w; }
    const uint32_t wp[4] = {up.x, up.y, up.z, up.w};
    float ss[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        uint32_t wbits = ((e & 1) ? wp[e >> 1] >> 16 : wp[e >> 1] & 0xffffu) << 16;
        if (MASTER) wbits += (uint32_t)(int32_t)(int16_t)((e & 1) ? wl[e >> 1] >> 16 : wl[e >> 1] & 0xffffu);
        const float d = ss[e] - __uint_as_float(wbits);
        const float t = omd * d;
        ss[e] = ss[e] - t;
    }
    *(float4*)(s + i) = make_float4(ss[0], ss[1], ss[2], ss[3]);
    *(float4*)(s + i + 4) = make_float4(ss[4], ss[5], ss[6], ss[7]);
}

__global__ __launch_bounds__(256) void ema_swap_in_kernel(bf16_t* __restrict__ p, int16_t* __restrict__ lo16, const float* __restrict__ s,
                                                          bf16_t* __restrict__ stash_p, int16_t* __restrict__ stash_lo, int zero_lo) {
    const long i = (long)blockIdx.x * 2048 + threadIdx.x * 8;
    const float4 s0 = *(const float4*)(s + i), s1 = *(const float4*)(s + i + 4);
    if (stash_p) *(uint4*)(stash_p + i) = *(const uint4*)(p + i);
    if (stash_lo) *(uint4*)(stash_lo + i) = *(const uint4*)(lo16 + i);
    const float ss[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
    uint32_t h[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) h[e] = f2bf(ss[e]);
    *(uint4*)(p + i) = make_uint4(h[0] | h[1] << 16, h[2] | h[3] << 16, h[4] | h[5] << 16, h[6] | h[7] << 16);
    if (zero_lo) *(uint4*)(lo16 + i) = make_uint4(0u, 0u, 0u, 0u);
}

}  // namespace

extern "C" int orv_ema_update(float* shadow, const void* p, const void* lo, long n, float one_minus_decay, void* stream) {
    ORV_REQUIRE(shadow && p, "orv_ema_update: null buffer (shadow fp32[n] and p bf16[n] are required; lo may be NULL)");
    ORV_REQUIRE(n > 0 && n % 2048 == 0 && n / 2048 <= 0x7fffffffL, "orv_ema_update: n=%ld must be a positive multiple of 2048 (pad every segment)", n);
    ORV_REQUIRE(orv_aligned(shadow, 16) && orv_aligned(p, 16) && orv_aligned(lo, 16),
                "orv_ema_update: shadow, p and lo must be 16-byte aligned (the kernel reads 16 bytes per access)");
    ORV_REQUIRE(one_minus_decay >= 0.f && one_minus_decay <= 1.f, "orv_ema_update: one_minus_decay=%g must lie in [0, 1]", (double)one_minus_decay);
    const dim3 grid((unsigned)(n / 2048)), block(256);
    if (lo)
        hipLaunchKernelGGL(ema_update_kernel<true>, grid, block, 0, (hipStream_t)stream, shadow, (const bf16_t*)p, (const int16_t*)lo,
                           one_minus_decay);
    else
        hipLaunchKernelGGL(ema_update_kernel<false>, grid, block, 0, (hipStream_t)stream, shadow, (const bf16_t*)p, (const int16_t*)nullptr,
                           one_minus_decay);
    return orv_check_launch("orv_ema_update");
}

extern "C" int orv_ema_swap_in(void* p, void* lo, const float* shadow, void* stash_p, void* stash_lo, long n, int zero_lo, void* stream) {
    ORV_REQUIRE(p && shadow, "orv_ema_swap_in: null buffer (p bf16[n] and shadow fp32[n] are required)");
    ORV_REQUIRE(n > 0 && n % 2048 == 0 && n / 2048 <= 0x7fffffffL, "orv_ema_swap_in: n=%ld must be a positive multiple of 2048 (pad every segment)", n);
    ORV_REQUIRE(lo || (!stash_lo && !zero_lo), "orv_ema_swap_in: stash_lo / zero_lo given without the low-half buffer lo");
    ORV_REQUIRE(!stash_lo || stash_p, "orv_ema_swap_in: stash_lo given without stash_p (the weights and their low halves are kept together)");
    ORV_REQUIRE(orv_aligned(p, 16) && orv_aligned(lo, 16) && orv_aligned(shadow, 16) && orv_aligned(stash_p, 16) && orv_aligned(stash_lo, 16),
                "orv_ema_swap_in: p, lo, shadow and the stash buffers must be 16-byte aligned (the kernel moves 16 bytes per access)");
    ORV_REQUIRE(stash_p != p && (!stash_lo || stash_lo != lo), "orv_ema_swap_in: a stash buffer aliases the buffer it keeps");
    hipLaunchKernelGGL(ema_swap_in_kernel, dim3((unsigned)(n / 2048)), dim3(256), 0, (hipStream_t)stream, (bf16_t*)p, (int16_t*)lo, shadow,
                       (bf16_t*)stash_p, (int16_t*)stash_lo, zero_lo ? 1 : 0);
    return orv_check_launch("orv_ema_swap_in");
}
