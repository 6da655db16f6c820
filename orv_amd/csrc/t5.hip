// T5 v1.1 text-encoder kernels (the reference encodes prompts with transformers' T5EncoderModel: orv/models/text_encoder.py:34,
// orv/models/cogvideox_control.py:1290-1299): relative-position-bias attention, RMS LayerNorm, gated-GELU product.
// The projections are orv_gemm_bf16 and the embedding is orv_gather_rows; see DESIGN.md §11.
#include "common.hpp"

namespace {

constexpr int T5_MAX_S = 512;   // one head's K and V^T (+ its bias row) stay in one workgroup's LDS: 280 * s_pad + 1024 bytes <= 160 KiB
constexpr int T5_KROW = 72;     // bf16 per K row in LDS (64 + 8: 144-byte rows keep ds_read_b128 16-byte aligned and off one bank column)
constexpr int T5_VPAD = 8;      // bf16 of padding per V^T row
constexpr float T5_LOG2E = 1.4426950408889634f;

struct T5AttnArgs {
    const bf16_t* qkv; long ld_qkv;
    const float* bias;
    bf16_t* out; long ld_out;
    int B, S, H, s_pad, nqb;
};

// One workgroup = one (batch, head, block of 64 queries); one wave = 16 queries; every wave sees all keys from LDS.
// Both products run transposed on v_mfma_f32_16x16x32_bf16 so that the query sits on the lane (column l & 15) everywhere:
//   S^T[key, query] = K . Q^T      A = K rows (ds_read_b128), B = Q^T (registers, loaded once)
//   O^T[d, query]  += V^T . P^T    A = V^T rows (2 x ds_read_b64), B = P^T = the S^T accumulators after the softmax, no lane movement:
// lane (query, g = l >> 4) holds keys kb + 4g .. 4g+3 of the first and kb + 16 + 4g .. +3 of the second 16-key tile of a 32-key chunk, and
// feeds them as contraction slots 8g .. 8g+7; the V^T operand is read in that same key order, so the sum over keys is the same sum.
// Online softmax over 32-key chunks: running row maximum (the true maximum: T5 scores are unbounded) and rescale.
__global__ __launch_bounds__(256) void t5_attn_kernel(const T5AttnArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int S = a.S, s_pad = a.s_pad, vrow = s_pad + T5_VPAD;
    bf16_t* Ks = (bf16_t*)smem;                    // [s_pad][T5_KROW]
    bf16_t* Vt = Ks + s_pad * T5_KROW;             // [64][vrow]
    float* bs = (float*)(Vt + 64 * vrow);          // [2 S - 1] of this head
    int item = blockIdx.x;
    const int qb = item % a.nqb;
    item /= a.nqb;
    const int h = item % a.H, b = item / a.H;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const bf16_t* qbase = a.qkv + (long)b * S * a.ld_qkv + h * 64;
    const bf16_t* kbase = qbase + a.H * 64;
    const bf16_t* vbase = kbase + a.H * 64;

    for (int i = tid; i < s_pad * 8; i += 256) {   // keys past S: zero rows (their P is 0; 0 * garbage could be NaN)
        const int key = i >> 3, c = i & 7;
        uint4 kk = make_uint4(0, 0, 0, 0), vv = make_uint4(0, 0, 0, 0);
        if (key < S) {
            kk = *(const uint4*)(kbase + (long)key * a.ld_qkv + c * 8);
            vv = *(const uint4*)(vbase + (long)key * a.ld_qkv + c * 8);
        }
        *(uint4*)(Ks + key * T5_KROW + c * 8) = kk;
        const uint32_t wv[4] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            Vt[(c * 8 + 2 * e) * vrow + key] = (bf16_t)(wv[e] & 0xffffu);
            Vt[(c * 8 + 2 * e + 1) * vrow + key] = (bf16_t)(wv[e] >> 16);
        }
    }
    for (int i = tid; i < 2 * S - 1; i += 256) bs[i] = a.bias[(long)h * (2 * S - 1) + i];
    __syncthreads();

    const int q0 = qb * 64 + w * 16;
    if (q0 >= S) return;                            // wave-uniform, after the only barrier
    const int qi = q0 + (lane & 15), g = lane >> 4;
    const bool qok = qi < S;
    const int qc = qok ? qi : S - 1;                // rows past S compute on a valid row and are not stored
    bf16x8 qf[2];
    {
        const bf16_t* qp = qbase + (long)qc * a.ld_qkv + g * 8;
        qf[0] = *(const bf16x8*)qp;
        qf[1] = *(const bf16x8*)(qp + 32);
    }
    const float* bq = bs + (S - 1 - qc);            // bq[j] = bias of (query qc, key j)
    float m = -INFINITY, l = 0.0f;
    f32x4 o[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};

    for (int kb = 0; kb < S; kb += 32) {
        f32x4 s[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const bf16_t* kp = Ks + (kb + t * 16 + (lane & 15)) * T5_KROW + g * 8;
            const bf16x8 k0 = *(const bf16x8*)kp, k1 = *(const bf16x8*)(kp + 32);
            f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k0, qf[0], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k1, qf[1], acc, 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int j = kb + t * 16 + g * 4 + i;
                acc[i] = j < S ? acc[i] + bq[j] : -INFINITY;
            }
            s[t] = acc;
        }
        float mx = fmaxf(fmaxf(fmaxf(s[0][0], s[0][1]), fmaxf(s[0][2], s[0][3])), fmaxf(fmaxf(s[1][0], s[1][1]), fmaxf(s[1][2], s[1][3])));
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));     // key kb < S is in every chunk: finite
        const float mn = fmaxf(m, mx);
        const float alpha = __builtin_amdgcn_exp2f((m - mn) * T5_LOG2E);   // first chunk: exp2(-inf) = 0
        float p[8], ps = 0.0f;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            p[i] = __builtin_amdgcn_exp2f((s[i >> 2][i & 3] - mn) * T5_LOG2E);
            ps += p[i];
        }
        ps += __shfl_xor(ps, 16, 64);
        ps += __shfl_xor(ps, 32, 64);
        l = l * alpha + ps;
        m = mn;
        union { uint32_t u[4]; bf16x8 v; } pf;
#pragma unroll
        for (int i = 0; i < 4; ++i) pf.u[i] = pack2bf(p[2 * i], p[2 * i + 1]);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            const bf16_t* vp = Vt + (dt * 16 + (lane & 15)) * vrow + kb + g * 4;
            union { uint2 u[2]; bf16x8 v; } vf;
            vf.u[0] = *(const uint2*)vp;
            vf.u[1] = *(const uint2*)(vp + 16);
            o[dt] = o[dt] * alpha;
            o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf.v, pf.v, o[dt], 0, 0, 0);
        }
    }
    if (qok) {
        const float inv = 1.0f / l;
        bf16_t* op = a.out + ((long)b * S + qi) * a.ld_out + h * 64 + g * 4;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
            *(uint2*)(op + dt * 16) = make_uint2(pack2bf(o[dt][0] * inv, o[dt][1] * inv), pack2bf(o[dt][2] * inv, o[dt][3] * inv));
    }
}

// y = w * bf16(x * rsqrt(mean(x^2) + eps)): one wave per row, 8 bf16 per lane and step; the second pass re-reads the row from cache
// (x and y may be the same buffer: no __restrict__ on them; a lane reads its chunk before it writes it, after the row's reduction)
__global__ __launch_bounds__(256) void t5_rmsnorm_kernel(const bf16_t* x, long ldx, const bf16_t* __restrict__ w, bf16_t* y, long ldy, int M,
                                                         int D, float eps) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= M) return;
    const bf16_t* xr = x + (long)row * ldx;
    bf16_t* yr = y + (long)row * ldy;
    float ss = 0.0f;
    for (int c = lane * 8; c < D; c += 512) {
        const uint4 u = *(const uint4*)(xr + c);
        const uint32_t wx[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float lo = bf2f(wx[e] & 0xffff), hi = bf2f(wx[e] >> 16);
            ss += lo * lo + hi * hi;
        }
    }
    ss = wave_sum(ss);
    const float r = 1.0f / sqrtf(ss / (float)D + eps);
    for (int c = lane * 8; c < D; c += 512) {
        const uint4 u = *(const uint4*)(xr + c), g = *(const uint4*)(w + c);
        const uint32_t wx[4] = {u.x, u.y, u.z, u.w}, wg[4] = {g.x, g.y, g.z, g.w};
        uint32_t o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float lo = bf2f(f2bf(bf2f(wx[e] & 0xffff) * r)), hi = bf2f(f2bf(bf2f(wx[e] >> 16) * r));
            o[e] = pack2bf(bf2f(wg[e] & 0xffff) * lo, bf2f(wg[e] >> 16) * hi);
        }
        *(uint4*)(yr + c) = make_uint4(o[0], o[1], o[2], o[3]);
    }
}

// out[m, f] = gelu_tanh(h[m, f]) * h[m, F + f], 8 columns per thread
__global__ __launch_bounds__(256) void geglu_kernel(const bf16_t* __restrict__ h, long ldh, bf16_t* __restrict__ out, long ldo, int M, int F) {
    const int nchunk = F >> 3;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)M * nchunk) return;
    const int r = (int)(i / nchunk), c = (int)(i % nchunk);
    const bf16_t* hp = h + (long)r * ldh + c * 8;
    const uint4 ua = *(const uint4*)hp, ub = *(const uint4*)(hp + F);
    const uint32_t wa[4] = {ua.x, ua.y, ua.z, ua.w}, wb[4] = {ub.x, ub.y, ub.z, ub.w};
    uint32_t o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e)
        o[e] = pack2bf(gelu_tanh(bf2f(wa[e] & 0xffff)) * bf2f(wb[e] & 0xffff), gelu_tanh(bf2f(wa[e] >> 16)) * bf2f(wb[e] >> 16));
    *(uint4*)(out + (long)r * ldo + c * 8) = make_uint4(o[0], o[1], o[2], o[3]);
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int orv_t5_attention_max_seq(void) { return T5_MAX_S; }

extern "C" int orv_t5_attention_fwd(const void* qkv, int ld_qkv, const float* bias_rel, void* out, int ld_out, int B, int S, int H,
                                    void* stream) {
    ORV_REQUIRE(qkv && bias_rel && out, "orv_t5_attention_fwd: null pointer");
    ORV_REQUIRE(B > 0 && S > 0 && H > 0, "orv_t5_attention_fwd: B, S, H must be positive (got %d, %d, %d)", B, S, H);
    ORV_REQUIRE(S <= T5_MAX_S, "orv_t5_attention_fwd: S = %d is above the supported maximum of %d keys (one head's K and V stay in LDS)", S,
                T5_MAX_S);
    ORV_REQUIRE(ld_qkv >= 3 * H * 64 && ld_qkv % 8 == 0 && ld_out >= H * 64 && ld_out % 8 == 0,
                "orv_t5_attention_fwd: ld_qkv >= 3 H 64, ld_out >= H 64, both multiples of 8 (got %d, %d, H = %d)", ld_qkv, ld_out, H);
    ORV_REQUIRE(aligned16(qkv) && aligned16(out) && ((uintptr_t)bias_rel & 3) == 0, "orv_t5_attention_fwd: qkv / out must be 16-byte aligned");
    const int nqb = (S + 63) / 64;
    ORV_REQUIRE((long)B * H * nqb < (1L << 31) && (long)B * S < (1L << 31), "orv_t5_attention_fwd: problem too large");
    T5AttnArgs a;
    a.qkv = (const bf16_t*)qkv, a.ld_qkv = ld_qkv, a.bias = bias_rel, a.out = (bf16_t*)out, a.ld_out = ld_out;
    a.B = B, a.S = S, a.H = H, a.s_pad = (S + 31) / 32 * 32, a.nqb = nqb;
    const int smem = a.s_pad * T5_KROW * 2 + 64 * (a.s_pad + T5_VPAD) * 2 + 2 * a.s_pad * 4;
    static int smem_max = 64 * 1024;
    if (smem > smem_max) {
        const int full = T5_MAX_S * T5_KROW * 2 + 64 * (T5_MAX_S + T5_VPAD) * 2 + 2 * T5_MAX_S * 4;
        if (hipFuncSetAttribute((const void*)t5_attn_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, full) != hipSuccess) {
            (void)hipGetLastError();
            orv_set_error("orv_t5_attention_fwd: the device refused %d bytes of LDS per workgroup", full);
            return ORV_EDEVICE;
        }
        smem_max = full;
    }
    hipLaunchKernelGGL(t5_attn_kernel, dim3((unsigned)(B * H * nqb)), dim3(256), smem, (hipStream_t)stream, a);
    return orv_check_launch("orv_t5_attention_fwd");
}

extern "C" int orv_t5_rmsnorm(const void* x, int ldx, const void* w, void* y, int ldy, int M, int D, float eps, void* stream) {
    ORV_REQUIRE(x && w && y, "orv_t5_rmsnorm: null pointer");
    ORV_REQUIRE(M > 0 && D > 0 && D % 64 == 0, "orv_t5_rmsnorm: M > 0 and D a positive multiple of 64 (got M = %d, D = %d)", M, D);
    ORV_REQUIRE(ldx >= D && ldy >= D && ldx % 8 == 0 && ldy % 8 == 0, "orv_t5_rmsnorm: ldx, ldy >= D and multiples of 8 (got %d, %d)", ldx, ldy);
    ORV_REQUIRE(aligned16(x) && aligned16(w) && aligned16(y), "orv_t5_rmsnorm: x / w / y must be 16-byte aligned");
    ORV_REQUIRE(eps >= 0.0f, "orv_t5_rmsnorm: eps must not be negative");
    hipLaunchKernelGGL(t5_rmsnorm_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, (long)ldx,
                       (const bf16_t*)w, (bf16_t*)y, (long)ldy, M, D, eps);
    return orv_check_launch("orv_t5_rmsnorm");
}

extern "C" int orv_geglu(const void* h, int ldh, void* out, int ldo, int M, int F, void* stream) {
    ORV_REQUIRE(h && out, "orv_geglu: null pointer");
    ORV_REQUIRE(M > 0 && F > 0 && F % 8 == 0, "orv_geglu: M > 0 and F a positive multiple of 8 (got M = %d, F = %d)", M, F);
    ORV_REQUIRE(ldh >= 2 * F && ldo >= F && ldh % 8 == 0 && ldo % 8 == 0, "orv_geglu: ldh >= 2 F, ldo >= F, both multiples of 8 (got %d, %d)",
                ldh, ldo);
    ORV_REQUIRE(aligned16(h) && aligned16(out), "orv_geglu: h / out must be 16-byte aligned");
    const long total = (long)M * (F / 8);
    ORV_REQUIRE((total + 255) / 256 < (1L << 31), "orv_geglu: problem too large");
    hipLaunchKernelGGL(geglu_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)h, (long)ldh,
                       (bf16_t*)out, (long)ldo, M, F);
    return orv_check_launch("orv_geglu");
}
