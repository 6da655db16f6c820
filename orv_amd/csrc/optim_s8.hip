// Opt-in block-scaled fp8 optimizer moments of the flat fused AdamW (orv_adamw_flat_s8, orv_state8_quantize, orv_state8_dequantize;
// FusedAdamW(state_precision="fp8")).  The fp32 moments m and v (8 bytes per element) become one byte each plus one
// scale byte per block of 256 consecutive flat elements (2 + 2/256 bytes per element).  THE FORMAT, bit for bit:
//
//   A block is 256 consecutive flat elements: 256 element bytes and one scale byte e + 127 (the e8m0 byte of mxfp8.hpp).
//        moment   element format   M   Emin   largest finite F
//        first    e4m3fn           3    -6    448
//        second   e5m2             2   -14    57344
//   Block exponent: e is the smallest integer with amax <= F 2^e, clamped to [-127, 127]; amax is taken over the FINITE new fp32 moments
//      of the block; an all-zero block or one without a finite element has byte 0 (e = -127).  From the fp32 bits amax = 1.m 2^(ef - 127):
//        e4m3: e = ef - 135 + (mant > 0x600000) ; e5m2: e = ef - 142 + (mant > 0x600000) ; a subnormal amax clamps to -127.
//   Scaling: y = x 2^-e, one fp32 product with subnormals kept; a = |y|.
//   Stochastic rounding to the element grid, in integers: E = max(floor(log2 a), Emin), s = 2^(E - M), w = floor(a / s 65536) (exact:
//      for a normal a the top M + 17 significand bits), n = (w + r) >> 16 with r a 16-bit integer; the stored magnitude is n s.  A carry
//      into the next binade, or from the subnormal range into the smallest normal, is just the next code; n s <= F always (F is on the
//      grid, a <= F).  The sign bit is that of x; a = 0 gives code 0 with the sign kept.  Unbiased to within 2^-16 of a grid step.
//   A non-finite moment stores 0x7F in both formats (NaN); the e5m2 codes 0x7C..0x7E are never written.
//   Random offsets: the hash of optim.hip (mix), on a second stream so that they are independent of the stochastic weight mode's r:
//        key2 = mix(hi32(i) + mix(step + mix(seed ^ 0x9E3779B9))) ; h = mix(lo32(i) ^ key2) ; r_m = h >> 16 ; r_v = h & 0xFFFF
//      `step` is the entry point's argument, i the flat index: launch geometry, wave, time and rank do not enter.
//   Dequantisation: code_value 2^e, exact in fp32 (e <= 120 for e4m3, e <= 113 for e5m2; the smallest value 2^-143 is a subnormal).
//
// THE UPDATE: dequantise m_old and v_old, then the fp32 formula and operation order of adamw_fp32 (optim.hip; contraction off, same clip,
// per-segment bias correction, decoupled decay, segment skip) with one change in the denominator:
//        w = w decay - lr (m ibc1) / (sqrt(max(v, vfloor) ibc2) + eps) ,  vfloor = 2^(e_v_old - 16)
// vfloor is the smallest positive value of the INCOMING second-moment grid of the block (a second moment that the e5m2 range of its block
// flushed to 0 while the first moment survived would otherwise divide by eps alone); 2^-143 for a never-written block: no effect.  The
// stored v is the un-floored one.  The weight uses the fresh fp32 m and v, not their quantised images, and is stored by `mode` as
// orv_adamw_flat_ex stores it (1 split fp32 master, 2 stochastic rounding; 0 here: nearest-even bf16 of the same fp32 result); then m
// and v are quantised and stored.  Inactive segments keep every byte: weights, lo, elements and scale bytes.
//
// Work split: a workgroup owns 2048 consecutive elements, 8 per lane (16-byte accesses on p, g, lo; 8-byte on m8, v8); a block is 32
// consecutive lanes (half a wave), its two maxima are DPP row reductions plus one exchange across the rows of 16 - no LDS.
#include "common.hpp"

#pragma clang fp contract(off)

namespace {

struct AdamwCoef {
    float b1, b2, omb1, omb2, lr, eps, decay, ibc1, ibc2, clip;
};

// the fp32 arithmetic of every mode of this file: adamw_fp32 of optim.hip with the floored second moment in the denominator
__device__ __forceinline__ float adamw_s8_fp32(float w, float g, float& m, float& v, float vfloor, const AdamwCoef& k) {
    const float gr = g * k.clip;
    m = k.b1 * m + k.omb1 * gr;
    v = k.b2 * v + k.omb2 * gr * gr;
    return w * k.decay - k.lr * (m * k.ibc1) / (sqrtf(fmaxf(v, vfloor) * k.ibc2) + k.eps);
}

__device__ __forceinline__ uint32_t mix32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

// per-launch part of the two keys (weight stream of optim.hip, state stream of this file); the rest depends on hi32(i) only
__device__ __forceinline__ uint32_t weight_key(uint32_t seed, uint32_t step, long i) {
    return mix32((uint32_t)((unsigned long)i >> 32) + mix32(step + mix32(seed)));
}
__device__ __forceinline__ uint32_t state_key(uint32_t seed, uint32_t step, long i) {
    return mix32((uint32_t)((unsigned long)i >> 32) + mix32(step + mix32(seed ^ 0x9E3779B9u)));
}

// M = 3: e4m3fn (first moment), M = 2: e5m2 (second moment)
template <int M> struct S8Fmt;
template <> struct S8Fmt<3> { static constexpr int kExpAdj = 135, kEmin = -6, kBias = 7; };
template <> struct S8Fmt<2> { static constexpr int kExpAdj = 142, kEmin = -14, kBias = 15; };

// Magnitude bits of x for the block maximum (unsigned order == order of the magnitudes).  CAREFUL: 0 for a non-finite x.  The fast
// variant keeps it, so a lane maximum >= 0x7f800000 tells that the wave holds a non-finite moment and must take the careful variant.
template <bool CAREFUL>
__device__ __forceinline__ uint32_t s8_abs(float x) {
    const uint32_t a = __float_as_uint(x) & 0x7fffffffu;
    return !CAREFUL || a < 0x7f800000u ? a : 0u;
}

// max over the 32 lanes of this lane's half wave, in every lane; all 64 lanes of the wave must execute it
__device__ __forceinline__ uint32_t s8_block_max(uint32_t v) {
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, true));     // quad_perm [1,0,3,2]
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, true));     // quad_perm [2,3,0,1]
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, true));    // row_half_mirror
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, true));    // row_mirror: the row of 16 agrees
    const auto r = __builtin_amdgcn_permlane16_swap(v, v, false, false);                    // rows 0<->1, 2<->3
    return max((uint32_t)r[0], (uint32_t)r[1]);
}

// block exponent e from the bits of the block's largest finite magnitude
template <int M>
__device__ __forceinline__ int s8_block_exp(uint32_t amax_bits) {
    const int ef = (int)(amax_bits >> 23);
    if (ef == 0) return -127;                                       // zero, nothing finite, or a subnormal amax (clamped)
    return max(ef - S8Fmt<M>::kExpAdj + ((amax_bits & 0x7fffffu) > 0x600000u ? 1 : 0), -127);
}

// 2^-e as an fp32, e in [-127, 120]: always a normal number
__device__ __forceinline__ float s8_inv_scale(int e) { return __uint_as_float((uint32_t)(127 - e) << 23); }

__device__ __forceinline__ uint2 s8_pack8(const uint32_t* b) {
    return make_uint2(b[0] | b[1] << 8 | b[2] << 16 | b[3] << 24, b[4] | b[5] << 8 | b[6] << 16 | b[7] << 24);
}

// x (fp32 moment) -> element byte of the block with inverse scale `inv`, stochastic rounding with the 16-bit offset r.
// CAREFUL = false assumes a finite x.
template <int M, bool CAREFUL>
__device__ __forceinline__ uint32_t s8_encode(float x, float inv, uint32_t r) {
    const uint32_t ux = __float_as_uint(x);
    const float y = x * inv;
    const uint32_t ua = __float_as_uint(y) & 0x7fffffffu;
    // normal range: the M + 17 significand bits above bit 6 - M plus r, carry into the exponent field = the next code
    const uint32_t nrm = ((ua + (r << (7 - M))) >> (23 - M)) - ((uint32_t)(127 - S8Fmt<M>::kBias) << M);
    // below 2^Emin: fixed step s = 2^(Emin - M), w = floor(a 2^(M - Emin + 16)) (the product is exact, the conversion truncates)
    const float up = __uint_as_float((uint32_t)(127 + M - S8Fmt<M>::kEmin + 16) << 23);
    const uint32_t sub = ((uint32_t)(__uint_as_float(ua) * up) + r) >> 16;
    const uint32_t mag = ua >= ((uint32_t)(127 + S8Fmt<M>::kEmin) << 23) ? nrm : sub;
    const uint32_t code = mag | ((ux >> 24) & 0x80u);
    return CAREFUL && (ux & 0x7fffffffu) >= 0x7f800000u ? 0x7fu : code;
}

// The two block exponents and the 8 + 8 element bytes of this lane's new moments (flat index i..i+7).  Every lane of the wave must
// execute it (cross-lane maxima).
template <bool CAREFUL>
__device__ __forceinline__ void s8_quantize_pair(const float* mm, const float* vv, long i, uint32_t key2, uint2& qm, uint2& qv, int& em,
                                                 int& ev) {
    uint32_t am = 0u, av = 0u;
#pragma unroll
    for (int e = 0; e < 8; ++e) { am = max(am, s8_abs<CAREFUL>(mm[e])); av = max(av, s8_abs<CAREFUL>(vv[e])); }
    em = s8_block_exp<3>(s8_block_max(am));
    ev = s8_block_exp<2>(s8_block_max(av));
    const float im = s8_inv_scale(em), iv = s8_inv_scale(ev);
    uint32_t bm[8], bv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const uint32_t h = mix32((uint32_t)(i + e) ^ key2);
        bm[e] = s8_encode<3, CAREFUL>(mm[e], im, h >> 16);
        bv[e] = s8_encode<2, CAREFUL>(vv[e], iv, h & 0xffffu);
    }
    qm = s8_pack8(bm);
    qv = s8_pack8(bv);
}

// 2^e as an fp32, e in [-127, 127] (2^-127 is the subnormal 0x00400000)
__device__ __forceinline__ float s8_scale(int e) { return __uint_as_float(e > -127 ? (uint32_t)(e + 127) << 23 : 0x00400000u); }

// 8 element bytes -> their values: the exact gfx950 conversions (OCP e4m3fn / e5m2), then one exact product with the block scale
template <int M>
__device__ __forceinline__ void s8_decode8(uint2 q, int e, float* out) {
    const uint32_t w[2] = {q.x, q.y};
    const float sc = s8_scale(e);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        if (M == 3) {
            const auto a = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[h], false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[h], true);
            out[4 * h] = a[0]; out[4 * h + 1] = a[1]; out[4 * h + 2] = b[0]; out[4 * h + 3] = b[1];
        } else {
            const auto a = __builtin_amdgcn_cvt_pk_f32_bf8((int)w[h], false), b = __builtin_amdgcn_cvt_pk_f32_bf8((int)w[h], true);
            out[4 * h] = a[0]; out[4 * h + 1] = a[1]; out[4 * h + 2] = b[0]; out[4 * h + 3] = b[1];
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) out[j] *= sc;                       // exact, also for e = -127 (subnormal operand and results kept)
}

// MODE 0: nearest-even bf16 weight; 1: split fp32 master (p + lo); 2: stochastic rounding of the weight.  10 + 2/256 bytes of traffic
// per element in modes 0 and 2 (14 in mode 1) against the 22 of the fp32-moment kernels.
// GROUPS: lr and wd are those of the segment's parameter group (orv_adamw_flat_s8_groups), picked once per workgroup with scalar selects
// from the by-value table, as in optim.hip.
template <int MODE, bool GROUPS>
__device__ __forceinline__ void adamw_flat_s8_body(bf16_t* __restrict__ p, int16_t* __restrict__ lo16, const bf16_t* __restrict__ g,
                                                   uint8_t* __restrict__ m8, uint8_t* __restrict__ v8, uint8_t* __restrict__ m_exp,
                                                   uint8_t* __restrict__ v_exp, const long* __restrict__ seg_start,
                                                   const uint8_t* __restrict__ active, int nseg, float lr, float b1, float b2, float eps,
                                                   float wd, float bc1, float bc2, const float* __restrict__ clip,
                                                   const int* __restrict__ seg_step, uint32_t seed, uint32_t step,
                                                   uint32_t common, const uint8_t* __restrict__ seg_group,
                                                   const orv_adamw_groups_t& groups) {
    const long e0 = (long)blockIdx.x * 2048;
    int lo = 0, hi = nseg - 1;                 // last segment with seg_start <= e0 (workgroup-uniform binary search)
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (seg_start[mid] <= e0) lo = mid; else hi = mid - 1; }
    // the group byte decides the branch together with the activity byte (a group outside the table: the segment is left alone), so the
    // two loads are in flight together instead of one behind the other
    const int gi = GROUPS ? seg_group[lo] : 0;
    if (!active[lo] | (gi >= ORV_ADAMW_MAX_GROUPS)) return;                   // uniform: every lane of a live wave reaches the cross-lane reductions below
    if (GROUPS) {
#pragma unroll
        for (int j = 0; j < ORV_ADAMW_MAX_GROUPS; ++j)
            if (gi == j) { lr = groups.lr[j]; wd = groups.weight_decay[j]; }
    }
    // one step count PER PARAMETER (bias correction), as in adamw_flat_kernel; a segment at the global count (the common case) takes the
    // host's corrections: two powf per lane are a fifth of this kernel's arithmetic, and the arithmetic, not the memory, bounds it
    // (`common` is the count bc1 / bc2 were made for: `step` itself in the parent; behind it after a skipped step, orv_adamw_flat_s8_groups)
    if (seg_step && (uint32_t)seg_step[lo] != common) {
        const float st = (float)seg_step[lo];
        bc1 = 1.f - powf(b1, st);
        bc2 = 1.f - powf(b2, st);
    }
    AdamwCoef k;
    k.b1 = b1; k.b2 = b2; k.omb1 = 1.f - b1; k.omb2 = 1.f - b2; k.lr = lr; k.eps = eps;
    k.decay = 1.f - lr * wd; k.ibc1 = 1.f / bc1; k.ibc2 = 1.f / bc2; k.clip = clip ? *clip : 1.f;
    const long i = e0 + threadIdx.x * 8;
    const long blk = (long)blockIdx.x * 8 + (threadIdx.x >> 5);
    const uint4 up = *(const uint4*)(p + i), ug = *(const uint4*)(g + i);
    const uint2 qm = *(const uint2*)(m8 + i), qv = *(const uint2*)(v8 + i);
    const int em_old = (int)m_exp[blk] - 127, ev_old = (int)v_exp[blk] - 127;
    float mm[8], vv[8];
    s8_decode8<3>(qm, em_old, mm);
    s8_decode8<2>(qv, ev_old, vv);
    const float vfloor = ldexpf(1.f, ev_old - 16);
    const uint32_t wp[4] = {up.x, up.y, up.z, up.w}, wg[4] = {ug.x, ug.y, ug.z, ug.w};
    uint32_t wl[4] = {0u, 0u, 0u, 0u};
    if (MODE == 1) { const uint4 ul = *(const uint4*)(lo16 + i); wl[0] = ul.x; wl[1] = ul.y; wl[2] = ul.z; wl[3] = ul.w; }
    // hi32(i) is the same for the whole workgroup (2^32 is a multiple of 2048): the keys are scalar work, off the per-element path
    const uint32_t key = MODE == 2 ? weight_key(seed, step, e0) : 0u;
    const uint32_t key2 = state_key(seed, step, e0);
    uint32_t np[8], nl[8], raw = 0u;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const uint32_t pb = (e & 1) ? wp[e >> 1] >> 16 : wp[e >> 1] & 0xffffu;
        const uint32_t gb = (e & 1) ? wg[e >> 1] >> 16 : wg[e >> 1] & 0xffffu;
        uint32_t wbits = pb << 16;
        if (MODE == 1) wbits += (uint32_t)(int32_t)(int16_t)((e & 1) ? wl[e >> 1] >> 16 : wl[e >> 1] & 0xffffu);
        const uint32_t u = __float_as_uint(adamw_s8_fp32(__uint_as_float(wbits), bf2f((bf16_t)gb), mm[e], vv[e], vfloor, k));
        raw = max(raw, max(s8_abs<false>(mm[e]), s8_abs<false>(vv[e])));
        const uint32_t a = u & 0x7fffffffu;
        if (a >= 0x7f800000u) {                // infinity / NaN: the matching bf16 (NaN kept quiet), no low half, no perturbation
            np[e] = (u >> 16) | (a > 0x7f800000u ? 0x40u : 0u);
            nl[e] = 0u;
        } else if (MODE == 1) {
            np[e] = (u + 0x8000u) >> 16;
            nl[e] = (u - (np[e] << 16)) & 0xffffu;
        } else if (MODE == 2) {
            const uint32_t t = u + (mix32((uint32_t)(i + e) ^ key) >> 16);
            np[e] = (t & 0x7fffffffu) >= 0x7f800000u ? ((u >> 16) & 0x8000u) | 0x7f7fu : t >> 16;
            nl[e] = 0u;
        } else {
            np[e] = (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
            nl[e] = 0u;
        }
    }
    *(uint4*)(p + i) = make_uint4(np[0] | np[1] << 16, np[2] | np[3] << 16, np[4] | np[5] << 16, np[6] | np[7] << 16);
    if (MODE == 1)
        *(uint4*)(lo16 + i) = make_uint4(nl[0] | nl[1] << 16, nl[2] | nl[3] << 16, nl[4] | nl[5] << 16, nl[6] | nl[7] << 16);
    uint2 nm, nv;
    int em, ev;
    // wave-uniform: the checks for non-finite moments are paid only by a wave that holds one
    if (__builtin_amdgcn_ballot_w64(raw >= 0x7f800000u)) s8_quantize_pair<true>(mm, vv, i, key2, nm, nv, em, ev);
    else s8_quantize_pair<false>(mm, vv, i, key2, nm, nv, em, ev);
    *(uint2*)(m8 + i) = nm;
    *(uint2*)(v8 + i) = nv;
    if ((threadIdx.x & 31) == 0) {             // one lane per block: plain vector byte stores
        m_exp[blk] = (uint8_t)(em + 127);
        v_exp[blk] = (uint8_t)(ev + 127);
    }
}

template <int MODE>
__global__ __launch_bounds__(256) void adamw_flat_s8_kernel(bf16_t* __restrict__ p, int16_t* __restrict__ lo16,
                                                            const bf16_t* __restrict__ g, uint8_t* __restrict__ m8,
                                                            uint8_t* __restrict__ v8, uint8_t* __restrict__ m_exp,
                                                            uint8_t* __restrict__ v_exp, const long* __restrict__ seg_start,
                                                            const uint8_t* __restrict__ active, int nseg, float lr, float b1,
                                                            float b2, float eps, float wd, float bc1, float bc2,
                                                            const float* __restrict__ clip, const int* __restrict__ seg_step,
                                                            uint32_t seed, uint32_t step) {
    adamw_flat_s8_body<MODE, false>(p, lo16, g, m8, v8, m_exp, v_exp, seg_start, active, nseg, lr, b1, b2, eps, wd, bc1, bc2, clip,
                                    seg_step, seed, step, step, nullptr, orv_adamw_groups_t{});
}

// the same body; lr and weight decay per parameter group
template <int MODE>
__global__ __launch_bounds__(256) void adamw_flat_s8_groups_kernel(bf16_t* __restrict__ p, int16_t* __restrict__ lo16,
                                                                   const bf16_t* __restrict__ g, uint8_t* __restrict__ m8,
                                                                   uint8_t* __restrict__ v8, uint8_t* __restrict__ m_exp,
                                                                   uint8_t* __restrict__ v_exp, const long* __restrict__ seg_start,
                                                                   const uint8_t* __restrict__ active, int nseg, float b1, float b2,
                                                                   float eps, float bc1, float bc2, const float* __restrict__ clip,
                                                                   const int* __restrict__ seg_step, uint32_t seed, uint32_t step,
                                                                   uint32_t common, const uint8_t* __restrict__ seg_group,
                                                                   const orv_adamw_groups_t groups) {
    adamw_flat_s8_body<MODE, true>(p, lo16, g, m8, v8, m_exp, v_exp, seg_start, active, nseg, 0.f, b1, b2, eps, 0.f, bc1, bc2, clip,
                                   seg_step, seed, step, common, seg_group, groups);
}

// fp32 -> the bytes adamw_flat_s8_kernel stores for these values at (seed, step, flat index); n % 256 == 0, so a block of 32 lanes is
// wholly inside or outside [0, n) and the outside lanes only take part in the reductions
template <int M>
__global__ __launch_bounds__(256) void state8_quantize_kernel(const float* __restrict__ x, uint8_t* __restrict__ q,
                                                              uint8_t* __restrict__ exps, long n, uint32_t seed, uint32_t step) {
    const long e0 = (long)blockIdx.x * 2048, i = e0 + threadIdx.x * 8;
    const bool in = i < n;
    float xx[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (in) {
        const float4 a = *(const float4*)(x + i), b = *(const float4*)(x + i + 4);
        xx[0] = a.x; xx[1] = a.y; xx[2] = a.z; xx[3] = a.w; xx[4] = b.x; xx[5] = b.y; xx[6] = b.z; xx[7] = b.w;
    }
    uint32_t am = 0u;
#pragma unroll
    for (int e = 0; e < 8; ++e) am = max(am, s8_abs<true>(xx[e]));
    const int ex = s8_block_exp<M>(s8_block_max(am));
    const float inv = s8_inv_scale(ex);
    const uint32_t key2 = state_key(seed, step, e0);
    uint32_t b[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const uint32_t h = mix32((uint32_t)(i + e) ^ key2);
        b[e] = s8_encode<M, true>(xx[e], inv, M == 3 ? h >> 16 : h & 0xffffu);
    }
    if (!in) return;
    *(uint2*)(q + i) = s8_pack8(b);
    if ((threadIdx.x & 31) == 0) exps[i >> 8] = (uint8_t)(ex + 127);
}

template <int M>
__global__ __launch_bounds__(256) void state8_dequantize_kernel(const uint8_t* __restrict__ q, const uint8_t* __restrict__ exps,
                                                                float* __restrict__ x, long n) {
    const long i = (long)blockIdx.x * 2048 + threadIdx.x * 8;
    if (i >= n) return;
    float xx[8];
    s8_decode8<M>(*(const uint2*)(q + i), (int)exps[i >> 8] - 127, xx);
    *(float4*)(x + i) = make_float4(xx[0], xx[1], xx[2], xx[3]);
    *(float4*)(x + i + 4) = make_float4(xx[4], xx[5], xx[6], xx[7]);
}

}  // namespace

extern "C" int orv_adamw_flat_s8(void* p, const void* g, unsigned char* m8, unsigned char* v8, unsigned char* m_exp,
                                 unsigned char* v_exp, long n, const long* seg_start, const unsigned char* seg_active,
                                 const int* seg_step, int nseg, float lr, float beta1, float beta2, float eps, float weight_decay,
                                 int step, const float* clip_coef, void* lo, int mode, unsigned seed, void* stream) {
    ORV_REQUIRE(mode >= 0 && mode <= 2, "orv_adamw_flat_s8: mode=%d (0 bf16, 1 split_fp32, 2 stochastic)", mode);
    ORV_REQUIRE(p && g && m8 && v8 && m_exp && v_exp && seg_start && seg_active && nseg > 0 && step > 0,
                "orv_adamw_flat_s8: bad arguments");
    ORV_REQUIRE(n > 0 && n % 2048 == 0, "orv_adamw_flat_s8: n=%ld must be a multiple of 2048 (pad every segment)", n);
    ORV_REQUIRE(mode != 1 || lo, "orv_adamw_flat_s8: mode 1 (split_fp32) needs the low-half buffer lo (int16[n])");
    const float bc1 = 1.f - powf(beta1, (float)step), bc2 = 1.f - powf(beta2, (float)step);
    const dim3 grid((unsigned)(n / 2048)), block(256);
#define ORV_S8_LAUNCH(MODE, LO)                                                                                                          \
    hipLaunchKernelGGL(adamw_flat_s8_kernel<MODE>, grid, block, 0, (hipStream_t)stream, (bf16_t*)p, (int16_t*)(LO), (const bf16_t*)g, m8, \
                       v8, m_exp, v_exp, seg_start, seg_active, nseg, lr, beta1, beta2, eps, weight_decay, bc1, bc2, clip_coef, seg_step, \
                       seed, (uint32_t)step)
    if (mode == 0) ORV_S8_LAUNCH(0, nullptr);
    else if (mode == 1) ORV_S8_LAUNCH(1, lo);
    else ORV_S8_LAUNCH(2, nullptr);
#undef ORV_S8_LAUNCH
    return orv_check_launch("orv_adamw_flat_s8");
}

extern "C" int orv_adamw_flat_s8_groups(void* p, const void* g, unsigned char* m8, unsigned char* v8, unsigned char* m_exp,
                                        unsigned char* v_exp, long n, const long* seg_start, const unsigned char* seg_active,
                                        const int* seg_step, int nseg, const unsigned char* seg_group, orv_adamw_groups_t groups,
                                        float beta1, float beta2, float eps, int step, int common_count, const float* clip_coef,
                                        void* lo, int mode, unsigned seed, void* stream) {
    ORV_REQUIRE(mode >= 0 && mode <= 2, "orv_adamw_flat_s8_groups: mode=%d (0 bf16, 1 split_fp32, 2 stochastic)", mode);
    ORV_REQUIRE(groups.ngroups >= 1 && groups.ngroups <= ORV_ADAMW_MAX_GROUPS, "orv_adamw_flat_s8_groups: ngroups=%d (supported: 1..%d)",
                groups.ngroups, ORV_ADAMW_MAX_GROUPS);
    ORV_REQUIRE(p && g && m8 && v8 && m_exp && v_exp && seg_start && seg_active && seg_group && nseg > 0 && step > 0,
                "orv_adamw_flat_s8_groups: bad arguments");
    ORV_REQUIRE(n > 0 && n % 2048 == 0, "orv_adamw_flat_s8_groups: n=%ld must be a multiple of 2048 (pad every segment)", n);
    ORV_REQUIRE(mode != 1 || lo, "orv_adamw_flat_s8_groups: mode 1 (split_fp32) needs the low-half buffer lo (int16[n])");
    // the host's bias corrections serve the segments at `common`: the global step, or the count the caller knows most segments are at
    const int common = common_count > 0 ? common_count : step;
    const float bc1 = 1.f - powf(beta1, (float)common), bc2 = 1.f - powf(beta2, (float)common);
    const dim3 grid((unsigned)(n / 2048)), block(256);
#define ORV_S8G_LAUNCH(MODE, LO)                                                                                                        \
    hipLaunchKernelGGL(adamw_flat_s8_groups_kernel<MODE>, grid, block, 0, (hipStream_t)stream, (bf16_t*)p, (int16_t*)(LO),              \
                       (const bf16_t*)g, m8, v8, m_exp, v_exp, seg_start, seg_active, nseg, beta1, beta2, eps, bc1, bc2, clip_coef,     \
                       seg_step, seed, (uint32_t)step, (uint32_t)common, seg_group, groups)
    if (mode == 0) ORV_S8G_LAUNCH(0, nullptr);
    else if (mode == 1) ORV_S8G_LAUNCH(1, lo);
    else ORV_S8G_LAUNCH(2, nullptr);
#undef ORV_S8G_LAUNCH
    return orv_check_launch("orv_adamw_flat_s8_groups");
}

extern "C" int orv_state8_quantize(const float* x, unsigned char* q, unsigned char* exps, long n, int format, unsigned seed, int step,
                                   void* stream) {
    ORV_REQUIRE(format == 0 || format == 1, "orv_state8_quantize: format=%d (0 first moment e4m3fn, 1 second moment e5m2)", format);
    ORV_REQUIRE(x && q && exps, "orv_state8_quantize: null buffer");
    ORV_REQUIRE(n > 0 && n % 256 == 0, "orv_state8_quantize: n=%ld must be a positive multiple of 256 (whole blocks)", n);
    const dim3 grid((unsigned)((n + 2047) / 2048)), block(256);
    if (format == 0)
        hipLaunchKernelGGL(state8_quantize_kernel<3>, grid, block, 0, (hipStream_t)stream, x, q, exps, n, seed, (uint32_t)step);
    else
        hipLaunchKernelGGL(state8_quantize_kernel<2>, grid, block, 0, (hipStream_t)stream, x, q, exps, n, seed, (uint32_t)step);
    return orv_check_launch("orv_state8_quantize");
}

extern "C" int orv_state8_dequantize(const unsigned char* q, const unsigned char* exps, float* x, long n, int format, void* stream) {
    ORV_REQUIRE(format == 0 || format == 1, "orv_state8_dequantize: format=%d (0 first moment e4m3fn, 1 second moment e5m2)", format);
    ORV_REQUIRE(q && exps && x, "orv_state8_dequantize: null buffer");
    ORV_REQUIRE(n > 0 && n % 256 == 0, "orv_state8_dequantize: n=%ld must be a positive multiple of 256 (whole blocks)", n);
    const dim3 grid((unsigned)((n + 2047) / 2048)), block(256);
    if (format == 0)
        hipLaunchKernelGGL(state8_dequantize_kernel<3>, grid, block, 0, (hipStream_t)stream, q, exps, x, n);
    else
        hipLaunchKernelGGL(state8_dequantize_kernel<2>, grid, block, 0, (hipStream_t)stream, q, exps, x, n);
    return orv_check_launch("orv_state8_dequantize");
}
