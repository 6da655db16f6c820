// orv_gemm_tn_skinny_bf16: C[P, Q] (+)= alpha * U[M, P]^T . V[M, Q] with min(P, Q) <= 128 - the weight gradients of a low-rank adapter
// (dB = c dY^T T with Q = rank, dA = dT^T X with P = rank), contracted over all M tokens.  The product is memory-bound (M = 12904, rank 64,
// D = 1920: 3.2 GFLOP over ~51 MB) and has only P Q / 64^2 output tiles, so the contraction is what gets split over the chip:
//   * a workgroup (4 waves) owns the whole small side (S = min(P, Q) = 16 NS columns) x 64 columns of the large side x one chunk of
//     contraction rows; wave w owns the 16-column block w of the large side and all NS blocks of the small side (NS accumulators).
//   * both operands are read row-major over the contraction rows, 16 bytes per lane, staged through registers into two LDS images of 64
//     rows (the loads of the next 64 rows are in flight while the MFMAs of the current ones run); fragments come from transposing reads
//     (ds_read_b64_tr_b16): k-step of 32 rows, lane (i16, g4) takes rows 4 g4 + (0..3) and 16 + 4 g4 + (0..3) of column i16 of its block -
//     the same k order on both operands.  Row strides are odd multiples of 32 bytes: the 8 rows a half-wave touches in one read fall into
//     8 different 32-byte bank groups.
//   * rows past the chunk's end are staged as zeros on both operands (nothing is masked afterwards); column blocks past the large side's
//     end are staged as zeros and not stored.
//   * chunk count and boundaries are a function of (M, P, Q) alone (skinny_plan).  Every chunk stores its fp32 partial [P, Q] into the
//     caller's scratch; a second kernel adds the partials in chunk order, scales by alpha, adds the old C (accumulate) and rounds once to
//     bf16.  No atomics: two runs give the same bits.
#include "common.hpp"

namespace {

constexpr int SK_KT = 64;          // contraction rows per LDS stage
constexpr int SK_LT = 64;          // large-side columns per workgroup
constexpr int SK_TARGET = 512;     // workgroups aimed at (two per CU)
constexpr int SK_MAXSPLIT = 32;
constexpr int SK_MINROWS = 128;    // a chunk is at least two stages, except the last

struct SkinnyPlan { int tiles, nsplit, rows; };

SkinnyPlan skinny_plan(int M, int P, int Q) {
    const int large = P <= Q ? Q : P;
    SkinnyPlan s;
    s.tiles = (large + SK_LT - 1) / SK_LT;
    int want = (SK_TARGET + s.tiles - 1) / s.tiles;
    if (want > SK_MAXSPLIT) want = SK_MAXSPLIT;
    if (want < 1) want = 1;
    int rows = (M + want - 1) / want;
    if (rows < SK_MINROWS) rows = SK_MINROWS;
    rows = (rows + SK_KT - 1) / SK_KT * SK_KT;
    s.rows = rows;
    s.nsplit = (M + rows - 1) / rows;
    return s;
}

struct SkinnyArgs {
    const bf16_t* S;  long lds_;    // small-side operand (S columns) and its row stride in elements
    const bf16_t* L;  long ldl;     // large-side operand
    float* part;                    // [nsplit, P, Q] fp32
    int M, P, Q, large, rows;
};

typedef short sk_v4s __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) char sk_lds_char;

__device__ __forceinline__ sk_v4s sk_tr(const char* a) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) sk_v4s*)(sk_lds_char*)(a));
}

constexpr int sk_stride(int bytes) { return ((bytes / 32) | 1) * 32; }      // odd multiple of 32 bytes >= bytes (bytes % 32 == 0)

// NS: 16-column blocks of the small side.  PSMALL: the small side is U (P = 16 NS), else V (Q = 16 NS).
template <int NS, bool PSMALL>
__global__ __launch_bounds__(256) void gemm_tn_skinny_kernel(const SkinnyArgs a) {
    constexpr int SB = NS * 32;                        // bytes of one small-side row
    constexpr int STS = sk_stride(SB), STL = sk_stride(SK_LT * 2);
    constexpr int CS = NS * 2;                         // 16-byte pieces per small-side row
    constexpr int NLS = (SK_KT * CS + 255) / 256;      // small-side pieces per thread and stage
    constexpr int NLL = SK_KT * 8 / 256;               // large-side pieces per thread and stage (2)
    __shared__ __attribute__((aligned(16))) char imgS[SK_KT * STS];
    __shared__ __attribute__((aligned(16))) char imgL[SK_KT * STL];

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int i16 = lane & 15, g4 = lane >> 4;
    const int col0 = blockIdx.x * SK_LT;               // first large-side column of this workgroup
    const int m0 = blockIdx.y * a.rows;
    const int m1 = min(m0 + a.rows, a.M);

    uint4 rs[NLS], rl[NLL];
    auto load = [&](int mb) {
#pragma unroll
        for (int j = 0; j < NLS; ++j) {
            const int i = t + j * 256, r = i / CS, c = i % CS;
            rs[j] = make_uint4(0, 0, 0, 0);
            if (i < SK_KT * CS && mb + r < m1) rs[j] = *(const uint4*)(a.S + (long)(mb + r) * a.lds_ + c * 8);
        }
#pragma unroll
        for (int j = 0; j < NLL; ++j) {
            const int i = t + j * 256, r = i >> 3, c = i & 7;
            rl[j] = make_uint4(0, 0, 0, 0);
            if (mb + r < m1 && col0 + c * 8 < a.large) rl[j] = *(const uint4*)(a.L + (long)(mb + r) * a.ldl + col0 + c * 8);
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int j = 0; j < NLS; ++j) {
            const int i = t + j * 256, r = i / CS, c = i % CS;
            if (i < SK_KT * CS) *(uint4*)(imgS + r * STS + c * 16) = rs[j];
        }
#pragma unroll
        for (int j = 0; j < NLL; ++j) {
            const int i = t + j * 256, r = i >> 3, c = i & 7;
            *(uint4*)(imgL + r * STL + c * 16) = rl[j];
        }
    };

    f32x4 acc[NS];
#pragma unroll
    for (int n = 0; n < NS; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};

    // lane's address inside a k-step: row 4 g4 + (i16 >> 2), 4 columns from 4 (i16 & 3) of its block; second read 16 rows further
    const char* const pS = imgS + (4 * g4 + (i16 >> 2)) * STS + (i16 & 3) * 8;
    const char* const pL = imgL + (4 * g4 + (i16 >> 2)) * STL + wave * 32 + (i16 & 3) * 8;

    load(m0);
    for (int mb = m0; mb < m1; mb += SK_KT) {
        __syncthreads();
        stage();
        __syncthreads();
        if (mb + SK_KT < m1) load(mb + SK_KT);
#pragma unroll
        for (int ks = 0; ks < SK_KT / 32; ++ks) {
            union { bf16x8 v; sk_v4s h[2]; } fl, fs;
            fl.h[0] = sk_tr(pL + ks * 32 * STL);
            fl.h[1] = sk_tr(pL + (ks * 32 + 16) * STL);
#pragma unroll
            for (int n = 0; n < NS; ++n) {
                fs.h[0] = sk_tr(pS + ks * 32 * STS + n * 32);
                fs.h[1] = sk_tr(pS + (ks * 32 + 16) * STS + n * 32);
                // D[row = q][col = p]: the lane ends up with 4 consecutive q of one p
                if constexpr (PSMALL) acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fl.v, fs.v, acc[n], 0, 0, 0);
                else acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fs.v, fl.v, acc[n], 0, 0, 0);
            }
        }
    }

    const int lcol = col0 + wave * 16;                 // this wave's large-side block (wave-uniform: in or out as a whole)
    if (lcol >= a.large) return;
    float* const part = a.part + (long)blockIdx.y * a.P * a.Q;
#pragma unroll
    for (int n = 0; n < NS; ++n) {
        const int p = PSMALL ? n * 16 + i16 : lcol + i16;
        const int q = (PSMALL ? lcol : n * 16) + 4 * g4;
        *(f32x4*)(part + (long)p * a.Q + q) = acc[n];
    }
}

__global__ __launch_bounds__(256) void gemm_tn_skinny_reduce_kernel(const float* __restrict__ part, bf16_t* __restrict__ C, long ldc, int P,
                                                                    int Q, int nsplit, float alpha, int accumulate) {
    const int q4n = Q >> 2;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)P * q4n) return;
    const int p = (int)(idx / q4n), q = (int)(idx % q4n) * 4;
    const long pq = (long)P * Q;
    const float* src = part + (long)p * Q + q;
    f32x4 s = *(const f32x4*)src;
    for (int c = 1; c < nsplit; ++c) {
        const f32x4 v = *(const f32x4*)(src + c * pq);
        s[0] += v[0]; s[1] += v[1]; s[2] += v[2]; s[3] += v[3];
    }
    s[0] *= alpha; s[1] *= alpha; s[2] *= alpha; s[3] *= alpha;
    bf16_t* cp = C + (long)p * ldc + q;
    if (accumulate) {
        const uint2 u = *(const uint2*)cp;
        s[0] += bf2f(u.x & 0xffff); s[1] += bf2f(u.x >> 16); s[2] += bf2f(u.y & 0xffff); s[3] += bf2f(u.y >> 16);
    }
    *(uint2*)cp = make_uint2(pack2bf(s[0], s[1]), pack2bf(s[2], s[3]));
}

template <int NS>
void skinny_launch(const SkinnyArgs& a, bool psmall, dim3 grid, hipStream_t st) {
    if (psmall) hipLaunchKernelGGL((gemm_tn_skinny_kernel<NS, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((gemm_tn_skinny_kernel<NS, false>), grid, dim3(256), 0, st, a);
}

}  // namespace

extern "C" long orv_gemm_tn_skinny_scratch(int M, int P, int Q) {
    if (M < 1 || P < 16 || Q < 16) return 0;
    return (long)skinny_plan(M, P, Q).nsplit * P * Q * 4;
}

extern "C" int orv_gemm_tn_skinny_bf16(const void* U, long ldu, const void* V, long ldv, void* C, long ldc, int M, int P, int Q, float alpha,
                                       int accumulate, void* scratch, void* stream) {
    ORV_REQUIRE(U && V && C, "orv_gemm_tn_skinny_bf16: null operand (U, V or C)");
    ORV_REQUIRE(scratch, "orv_gemm_tn_skinny_bf16: null scratch (orv_gemm_tn_skinny_scratch(M, P, Q) bytes)");
    ORV_REQUIRE(M >= 1, "orv_gemm_tn_skinny_bf16: M=%d must be at least 1", M);
    ORV_REQUIRE(P >= 16 && P % 16 == 0, "orv_gemm_tn_skinny_bf16: P=%d must be a positive multiple of 16", P);
    ORV_REQUIRE(Q >= 16 && Q % 16 == 0, "orv_gemm_tn_skinny_bf16: Q=%d must be a positive multiple of 16", Q);
    ORV_REQUIRE((P < Q ? P : Q) <= 128, "orv_gemm_tn_skinny_bf16: min(P, Q)=%d must be at most 128 (P=%d Q=%d)", P < Q ? P : Q, P, Q);
    ORV_REQUIRE(ldu % 8 == 0 && ldu >= P, "orv_gemm_tn_skinny_bf16: ldu=%ld must be a multiple of 8 (16-byte rows) and at least P=%d", ldu, P);
    ORV_REQUIRE(ldv % 8 == 0 && ldv >= Q, "orv_gemm_tn_skinny_bf16: ldv=%ld must be a multiple of 8 (16-byte rows) and at least Q=%d", ldv, Q);
    ORV_REQUIRE(ldc % 8 == 0 && ldc >= Q, "orv_gemm_tn_skinny_bf16: ldc=%ld must be a multiple of 8 (16-byte rows) and at least Q=%d", ldc, Q);
    ORV_REQUIRE(((uintptr_t)U & 15) == 0 && ((uintptr_t)V & 15) == 0 && ((uintptr_t)C & 15) == 0 && ((uintptr_t)scratch & 15) == 0,
                "orv_gemm_tn_skinny_bf16: U, V, C and scratch must be 16-byte aligned");
    const SkinnyPlan pl = skinny_plan(M, P, Q);
    const bool psmall = P <= Q;
    SkinnyArgs a;
    a.S = (const bf16_t*)(psmall ? U : V); a.lds_ = psmall ? ldu : ldv;
    a.L = (const bf16_t*)(psmall ? V : U); a.ldl = psmall ? ldv : ldu;
    a.part = (float*)scratch;
    a.M = M; a.P = P; a.Q = Q; a.large = psmall ? Q : P; a.rows = pl.rows;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(pl.tiles, pl.nsplit);
    switch ((psmall ? P : Q) / 16) {
        case 1: skinny_launch<1>(a, psmall, grid, st); break;
        case 2: skinny_launch<2>(a, psmall, grid, st); break;
        case 3: skinny_launch<3>(a, psmall, grid, st); break;
        case 4: skinny_launch<4>(a, psmall, grid, st); break;
        case 5: skinny_launch<5>(a, psmall, grid, st); break;
        case 6: skinny_launch<6>(a, psmall, grid, st); break;
        case 7: skinny_launch<7>(a, psmall, grid, st); break;
        default: skinny_launch<8>(a, psmall, grid, st); break;
    }
    int rc = orv_check_launch("orv_gemm_tn_skinny_bf16");
    if (rc != ORV_OK) return rc;
    const long n4 = (long)P * (Q / 4);
    hipLaunchKernelGGL(gemm_tn_skinny_reduce_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, (const float*)scratch, (bf16_t*)C, ldc,
                       P, Q, pl.nsplit, alpha, accumulate != 0);
    return orv_check_launch("orv_gemm_tn_skinny_bf16");
}
