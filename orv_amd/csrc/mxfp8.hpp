// OCP MXFP8 (include/orv_mi355.h "MXFP8"): a row of K values is cut into blocks of 32 consecutive elements; a block is 32 e4m3fn
// bytes plus one e8m0 scale byte 2^e, e the smallest integer with amax / 2^e <= 448, clamped to [-127, 127] (amax == 0: e = 0,
// byte 0x7F); element = x / 2^e rounded to nearest-even in e4m3fn, saturated to +-448.  The input is always the bf16 value.
//
// Work split shared by every producer: one lane owns 8 consecutive elements (one 16-byte bf16 chunk), the four lanes of an aligned
// lane quad own one 32-element block, so the block maximum is two DPP steps inside the quad.
#pragma once
#include "common.hpp"

// block exponent e of the rule above from the block's largest magnitude (a bf16 value, so exact in fp32)
__device__ __forceinline__ int mx_block_exp(float amax) {
    const uint32_t u = __float_as_uint(amax);
    const int ef = (int)(u >> 23) & 0xff;
    if (ef == 0) return u ? -127 : 0;                       // zero block: 2^0; subnormal amax needs e < -127: clamped
    // amax = 1.m * 2^(ef - 127); amax / 2^e <= 448 = 1.75 * 2^8  <=>  e >= ef - 135 (+1 when 1.m > 1.75)
    const int e = ef - 135 + ((u & 0x7fffffu) > 0x600000u ? 1 : 0);
    return min(max(e, -127), 127);
}

// 2^-e as an fp32 (e in [-127, 127]; 2^-127 is the fp32 subnormal 0x00400000)
__device__ __forceinline__ float mx_inv_scale(int e) {
    return e == 127 ? __uint_as_float(0x00400000u) : __uint_as_float((uint32_t)(127 - e) << 23);
}

// fp32 -> e4m3fn byte, round to nearest-even, saturating to +-448 (finite inputs)
__device__ __forceinline__ uint32_t mx_e4m3(float y) {
    const uint32_t sign = (__float_as_uint(y) >> 24) & 0x80u;
    const float a = fabsf(y);
    uint32_t enc;
    if (a < 0.015625f) {                                    // below 2^-6: the subnormal grid of 2^-9 steps (8 steps = 0x08 = 2^-6)
        enc = (uint32_t)__builtin_rintf(a * 512.0f);
    } else {
        uint32_t u = __float_as_uint(a);
        u += 0x7ffffu + ((u >> 20) & 1u);                   // round the fp32 mantissa to 3 bits, ties to even
        enc = ((((u >> 23) - 120u) << 3) | ((u >> 20) & 7u));
    }
    return sign | min(enc, 0x7eu);
}

// max over the four lanes of this lane's aligned quad (DPP quad_perm, no LDS)
__device__ __forceinline__ float mx_quad_max(float v) {
    v = fmaxf(v, __uint_as_float(__builtin_amdgcn_update_dpp(0, __float_as_uint(v), 0xB1, 0xF, 0xF, true)));   // [1,0,3,2]
    v = fmaxf(v, __uint_as_float(__builtin_amdgcn_update_dpp(0, __float_as_uint(v), 0x4E, 0xF, 0xF, true)));   // [2,3,0,1]
    return v;
}

// Quantise the 8 bf16 values of this lane (packed as in a 16-byte chunk); the lane quad forms one block.  Every lane of the wave
// must execute this (DPP); q = the lane's 8 e4m3 bytes, scale = the block's e8m0 byte (the same in all four lanes).
__device__ __forceinline__ void mx_quantize8(const uint4 bf, uint2& q, uint32_t& scale) {
    const uint32_t w[4] = {bf.x, bf.y, bf.z, bf.w};
    float v[8];
    float amax = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        v[2 * e] = bf2f(w[e] & 0xffff);
        v[2 * e + 1] = bf2f(w[e] >> 16);
        amax = fmaxf(amax, fmaxf(fabsf(v[2 * e]), fabsf(v[2 * e + 1])));
    }
    const int ex = mx_block_exp(mx_quad_max(amax));
    const float inv = mx_inv_scale(ex);
    uint32_t b[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) b[e] = mx_e4m3(v[e] * inv);
    q.x = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
    q.y = b[4] | (b[5] << 8) | (b[6] << 16) | (b[7] << 24);
    scale = (uint32_t)(ex + 127);
}

// Store of one lane's share: 8 bytes of q at element `c8 * 8` of the row, the scale byte by the first lane of the quad.
__device__ __forceinline__ void mx_store8(uint8_t* qrow, uint8_t* srow, int c8, uint2 q, uint32_t scale) {
    *(uint2*)(qrow + (long)c8 * 8) = q;
    if ((c8 & 3) == 0) srow[c8 >> 2] = (uint8_t)scale;
}
