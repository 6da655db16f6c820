// Fused Prodigy (the learning-rate-free optimizer; FusedProdigy) on the flat layout of the fused AdamW: every parameter a
// segment padded to 2048 elements, one workgroup of 256 lanes per 2048-element chunk, 8 elements per lane, 16-byte accesses.  The weight is
// the split fp32 master of orv_adamw_flat_ex mode 1 (optim.hip): master_bits = (p_bits << 16) + sign_extend(lo), written back as
// p_bits = (master_bits + 0x8000) >> 16, lo = master_bits - (p_bits << 16); a non-finite master writes the matching bf16 (NaN quiet), lo = 0.
//
// One step is three stream-ordered launches; every scalar of the step-size estimate stays on the device, in `state` (fp64[8]):
//      [0] d   [1] d_max   [2] d_numerator   [3] d_denom   [4] d_hat   [5] k (completed updates)   [6] dlr of this step   [7] skip flag
//
//   1. orv_prodigy_moments   per element of an active segment, g the clipped gradient, w the master, d and k the OLD state:
//          bc = use_bias_correction ? sqrt(1 - b2^(k+1)) / (1 - b1^(k+1)) : 1 ;  dlr = d lr bc                      (fp64, then rounded to fp32)
//          p0 = bf16 part of w where seg_step == 1 (first update of the parameter), else read
//          g += wd w                        (coupled decay only)
//          num_lane += ((d / d0) dlr g) (p0 - w)
//          m = b1 m + (d (1 - b1)) g ;  v = b2 v + ((d d (1 - b2)) g) g ;  s = b3 s + ((d / d0) (safeguard ? d : dlr)) g ;  den_lane += |s|
//      The chunk's two sums go lane -> wave -> the four waves in fp32 and are stored as ONE fp64 pair partials[2 chunk .. 2 chunk + 1]; the
//      chunks of an inactive segment store zeros and touch nothing else.  No atomics: the sums do not depend on arrival order.
//   2. orv_prodigy_recurrence   one workgroup of 512 lanes: lane t adds the pairs of chunks t, t + 512, ... in ascending order, the 512 lane
//      sums are added in runs of 32 in lane order and the 16 run sums in order (fp64 throughout, a fixed order); then num = b3 d_numerator + sum, den = sum and
//          den == 0: skip = 1 and d, d_max, d_numerator, d_hat, k stay;  else  d_hat = d_coef num / den ; if (d == d0) d = max(d, d_hat) ;
//          d_max = max(d_max, d_hat) ; d = min(d_max, d growth_rate) ; d_numerator = num ; k += 1 ; skip = 0.        d_denom and dlr are stored.
//   3. orv_prodigy_update   nothing when skip is set; else per element of an active segment, d the NEW one, dlr that of launch 1:
//          w -= (wd dlr) w                  (decoupled decay only) ;   w -= (dlr m) / (sqrt(v) + d eps)
#include "common.hpp"

#pragma clang fp contract(off)

namespace {

enum { PS_D = 0, PS_DMAX, PS_DNUM, PS_DDEN, PS_DHAT, PS_K, PS_DLR, PS_SKIP };

// dlr of the step that starts from `state`, the same expression in launch 1 and launch 2 (which stores it for launch 3)
__device__ __forceinline__ double prodigy_dlr(const double* __restrict__ state, float lr, float b1, float b2, int use_bc) {
    double bc = 1.0;
    if (use_bc) {
        const double k1 = state[PS_K] + 1.0;
        bc = sqrt(1.0 - pow((double)b2, k1)) / (1.0 - pow((double)b1, k1));
    }
    return state[PS_D] * (double)lr * bc;
}

// last segment with seg_start <= e0 (wave-uniform binary search, as in adamw_flat_ex_kernel)
__device__ __forceinline__ int segment_of(const long* __restrict__ seg_start, int nseg, long e0) {
    int lo = 0, hi = nseg - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (seg_start[mid] <= e0) lo = mid; else hi = mid - 1; }
    return lo;
}

__device__ __forceinline__ uint32_t half_of(const uint32_t* w, int e) { return (e & 1) ? w[e >> 1] >> 16 : w[e >> 1] & 0xffffu; }

__global__ __launch_bounds__(256) void prodigy_moments_kernel(const bf16_t* __restrict__ p, const int16_t* __restrict__ lo16,
                                                              const bf16_t* __restrict__ g, bf16_t* __restrict__ p0,
                                                              float* __restrict__ m, float* __restrict__ v, float* __restrict__ s,
                                                              const long* __restrict__ seg_start, const uint8_t* __restrict__ active,
                                                              const int* __restrict__ seg_step, int nseg,
                                                              const double* __restrict__ state, double* __restrict__ partials, float lr,
                                                              float b1, float b2, float b3, float wd, int decouple, int safeguard,
                                                              int use_bc, double d0, const float* __restrict__ clip) {
    __shared__ float red[8];
    const long e0 = (long)blockIdx.x * 2048;
    const int seg = segment_of(seg_start, nseg, e0);
    if (!active[seg]) {
        if (threadIdx.x == 0) { partials[2 * (long)blockIdx.x] = 0.0; partials[2 * (long)blockIdx.x + 1] = 0.0; }
        return;
    }
    const bool capture = seg_step[seg] == 1;
    const double dd = state[PS_D], dlr64 = prodigy_dlr(state, lr, b1, b2, use_bc), ratio = dd / d0;
    const float d = (float)dd;
    const float c_num = (float)(ratio * dlr64), c_m = d * (1.f - b1), c_v = d * d * (1.f - b2);
    const float c_s = (float)(ratio * (safeguard ? dd : dlr64)), cl = clip ? *clip : 1.f;
    const bool coupled = wd != 0.f && !decouple;

    const long i = e0 + threadIdx.x * 8;
    const uint4 up = *(const uint4*)(p + i), ul = *(const uint4*)(lo16 + i), ug = *(const uint4*)(g + i);
    uint4 u0 = up;                              // first update: p0 is the bf16 part of the master
    if (!capture) u0 = *(const uint4*)(p0 + i);
    const float4 m0 = *(const float4*)(m + i), m1 = *(const float4*)(m + i + 4), v0 = *(const float4*)(v + i), v1 = *(const float4*)(v + i + 4);
    const float4 s0 = *(const float4*)(s + i), s1 = *(const float4*)(s + i + 4);
    float mm[8] = {m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, m1.z, m1.w}, vv[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
    float ss[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
    const uint32_t wp[4] = {up.x, up.y, up.z, up.w}, wl[4] = {ul.x, ul.y, ul.z, ul.w}, wg[4] = {ug.x, ug.y, ug.z, ug.w};
    const uint32_t w0[4] = {u0.x, u0.y, u0.z, u0.w};
    float num = 0.f, den = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float w = __uint_as_float((half_of(wp, e) << 16) + (uint32_t)(int32_t)(int16_t)half_of(wl, e));
        float gr = bf2f((bf16_t)half_of(wg, e)) * cl;
        if (coupled) gr = gr + wd * w;
        num += (c_num * gr) * (bf2f((bf16_t)half_of(w0, e)) - w);
        mm[e] = b1 * mm[e] + c_m * gr;
        vv[e] = b2 * vv[e] + (c_v * gr) * gr;
        ss[e] = b3 * ss[e] + c_s * gr;
        den += fabsf(ss[e]);
    }
    *(float4*)(m + i) = make_float4(mm[0], mm[1], mm[2], mm[3]); *(float4*)(m + i + 4) = make_float4(mm[4], mm[5], mm[6], mm[7]);
    *(float4*)(v + i) = make_float4(vv[0], vv[1], vv[2], vv[3]); *(float4*)(v + i + 4) = make_float4(vv[4], vv[5], vv[6], vv[7]);
    *(float4*)(s + i) = make_float4(ss[0], ss[1], ss[2], ss[3]); *(float4*)(s + i + 4) = make_float4(ss[4], ss[5], ss[6], ss[7]);
    if (capture) *(uint4*)(p0 + i) = up;
    // lane -> wave -> the four waves, a fixed order: the pair depends on the inputs only
    num = wave_sum_valu(num);
    den = wave_sum_valu(den);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[wave] = num; red[4 + wave] = den; }
    __syncthreads();
    if (threadIdx.x == 0) {
        partials[2 * (long)blockIdx.x] = (double)(((red[0] + red[1]) + red[2]) + red[3]);
        partials[2 * (long)blockIdx.x + 1] = (double)(((red[4] + red[5]) + red[6]) + red[7]);
    }
}

// ONE workgroup of 512 lanes; at the 2B model's 825 k chunks (13 MB of pairs) the loop is bound by the latency of its loads, so eight
// independent 16-byte loads are in flight per lane - the additions stay in ascending chunk order, the sum is the same as without unrolling
__global__ __launch_bounds__(512) void prodigy_recurrence_kernel(double* __restrict__ state, const double* __restrict__ partials,
                                                                 long nchunks, float lr, float b1, float b2, float b3, int use_bc,
                                                                 double d0, double d_coef, double growth) {
    __shared__ double red[1024], red2[32];
    double num = 0.0, den = 0.0;
    long c = threadIdx.x;
    for (; c + 7 * 512 < nchunks; c += 8 * 512) {
        double2 q[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) q[j] = *(const double2*)(partials + 2 * (c + j * 512));
#pragma unroll
        for (int j = 0; j < 8; ++j) { num += q[j].x; den += q[j].y; }
    }
    for (; c < nchunks; c += 512) {
        const double2 pr = *(const double2*)(partials + 2 * c);
        num += pr.x;
        den += pr.y;
    }
    red[threadIdx.x] = num;
    red[512 + threadIdx.x] = den;
    __syncthreads();
    if (threadIdx.x < 16) {                    // the 512 lane sums in runs of 32, lane order
        num = 0.0; den = 0.0;
        for (int t = 0; t < 32; ++t) { num += red[threadIdx.x * 32 + t]; den += red[512 + threadIdx.x * 32 + t]; }
        red2[threadIdx.x] = num;
        red2[16 + threadIdx.x] = den;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    num = 0.0; den = 0.0;
    for (int t = 0; t < 16; ++t) { num += red2[t]; den += red2[16 + t]; }
    double d = state[PS_D];
    state[PS_DLR] = prodigy_dlr(state, lr, b1, b2, use_bc);          // from the OLD d and k
    state[PS_DDEN] = den;
    if (den == 0.0) {                          // nothing has ever had a non-zero gradient: no estimate, no weight update, no count
        state[PS_SKIP] = 1.0;
        return;
    }
    num = (double)b3 * state[PS_DNUM] + num;
    const double d_hat = d_coef * num / den;
    if (d == d0) d = fmax(d, d_hat);
    const double d_max = fmax(state[PS_DMAX], d_hat);
    state[PS_D] = fmin(d_max, d * growth);
    state[PS_DMAX] = d_max;
    state[PS_DNUM] = num;
    state[PS_DHAT] = d_hat;
    state[PS_K] = state[PS_K] + 1.0;
    state[PS_SKIP] = 0.0;
}

__global__ __launch_bounds__(256) void prodigy_update_kernel(bf16_t* __restrict__ p, int16_t* __restrict__ lo16,
                                                             const float* __restrict__ m, const float* __restrict__ v,
                                                             const long* __restrict__ seg_start, const uint8_t* __restrict__ active,
                                                             int nseg, const double* __restrict__ state, float eps, float wd,
                                                             int decouple) {
    if (state[PS_SKIP] != 0.0) return;
    const long e0 = (long)blockIdx.x * 2048;
    if (!active[segment_of(seg_start, nseg, e0)]) return;
    const float d = (float)state[PS_D], dlr = (float)state[PS_DLR];
    const float deps = d * eps, wdlr = wd * dlr;
    const bool decay = wd != 0.f && decouple;
    const long i = e0 + threadIdx.x * 8;
    const uint4 up = *(const uint4*)(p + i), ul = *(const uint4*)(lo16 + i);
    const float4 m0 = *(const float4*)(m + i), m1 = *(const float4*)(m + i + 4), v0 = *(const float4*)(v + i), v1 = *(const float4*)(v + i + 4);
    const float mm[8] = {m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, m1.z, m1.w}, vv[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
    const uint32_t wp[4] = {up.x, up.y, up.z, up.w}, wl[4] = {ul.x, ul.y, ul.z, ul.w};
    uint32_t np[8], nl[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        float w = __uint_as_float((half_of(wp, e) << 16) + (uint32_t)(int32_t)(int16_t)half_of(wl, e));
        if (decay) w = w - wdlr * w;
        w = w - (dlr * mm[e]) / (sqrtf(vv[e]) + deps);
        const uint32_t u = __float_as_uint(w), a = u & 0x7fffffffu;
        if (a >= 0x7f800000u) {                // infinity / NaN: the matching bf16 (NaN kept quiet), no low half
            np[e] = (u >> 16) | (a > 0x7f800000u ? 0x40u : 0u);
            nl[e] = 0u;
        } else {
            np[e] = (u + 0x8000u) >> 16;
            nl[e] = (u - (np[e] << 16)) & 0xffffu;
        }
    }
    *(uint4*)(p + i) = make_uint4(np[0] | np[1] << 16, np[2] | np[3] << 16, np[4] | np[5] << 16, np[6] | np[7] << 16);
    *(uint4*)(lo16 + i) = make_uint4(nl[0] | nl[1] << 16, nl[2] | nl[3] << 16, nl[4] | nl[5] << 16, nl[6] | nl[7] << 16);
}

}  // namespace

extern "C" int orv_prodigy_moments(const void* p, const void* lo, const void* g, void* p0, float* m, float* v, float* s, long n,
                                   const long* seg_start, const unsigned char* seg_active, const int* seg_step, int nseg,
                                   const double* state, double* partials, float lr, float beta1, float beta2, float beta3,
                                   float weight_decay, int decouple, int safeguard_warmup, int use_bias_correction, double d0,
                                   const float* clip_coef, void* stream) {
    ORV_REQUIRE(p && lo && g && p0 && m && v && s && seg_start && seg_active && seg_step && state && partials && nseg > 0,
                "orv_prodigy_moments: bad arguments (a null buffer, or nseg=%d)", nseg);
    ORV_REQUIRE(n > 0 && n % 2048 == 0, "orv_prodigy_moments: n=%ld must be a multiple of 2048 (pad every segment)", n);
    ORV_REQUIRE(d0 > 0.0, "orv_prodigy_moments: d0=%g must be greater than 0", d0);
    hipLaunchKernelGGL(prodigy_moments_kernel, dim3((unsigned)(n / 2048)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)p,
                       (const int16_t*)lo, (const bf16_t*)g, (bf16_t*)p0, m, v, s, seg_start, seg_active, seg_step, nseg, state, partials,
                       lr, beta1, beta2, beta3, weight_decay, decouple, safeguard_warmup, use_bias_correction, d0, clip_coef);
    return orv_check_launch("orv_prodigy_moments");
}

extern "C" int orv_prodigy_recurrence(double* state, const double* partials, long nchunks, float lr, float beta1, float beta2,
                                      float beta3, int use_bias_correction, double d0, double d_coef, double growth_rate, void* stream) {
    ORV_REQUIRE(state && partials && nchunks > 0, "orv_prodigy_recurrence: bad arguments (a null buffer, or nchunks=%ld)", nchunks);
    ORV_REQUIRE(d0 > 0.0, "orv_prodigy_recurrence: d0=%g must be greater than 0", d0);
    hipLaunchKernelGGL(prodigy_recurrence_kernel, dim3(1), dim3(512), 0, (hipStream_t)stream, state, partials, nchunks, lr, beta1, beta2,
                       beta3, use_bias_correction, d0, d_coef, growth_rate);
    return orv_check_launch("orv_prodigy_recurrence");
}

extern "C" int orv_prodigy_update(void* p, void* lo, const float* m, const float* v, long n, const long* seg_start,
                                  const unsigned char* seg_active, int nseg, const double* state, float eps, float weight_decay,
                                  int decouple, void* stream) {
    ORV_REQUIRE(p && lo && m && v && seg_start && seg_active && state && nseg > 0,
                "orv_prodigy_update: bad arguments (a null buffer, or nseg=%d)", nseg);
    ORV_REQUIRE(n > 0 && n % 2048 == 0, "orv_prodigy_update: n=%ld must be a multiple of 2048 (pad every segment)", n);
    ORV_REQUIRE(eps > 0.f, "orv_prodigy_update: eps=%g must be greater than 0 (a zero second moment divides by d eps)", (double)eps);
    hipLaunchKernelGGL(prodigy_update_kernel, dim3((unsigned)(n / 2048)), dim3(256), 0, (hipStream_t)stream, (bf16_t*)p, (int16_t*)lo, m, v,
                       seg_start, seg_active, nseg, state, eps, weight_decay, decouple);
    return orv_check_launch("orv_prodigy_update");
}
