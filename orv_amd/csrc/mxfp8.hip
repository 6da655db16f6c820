// MXFP8 inference GEMMs for gfx950 (opt-in mode, CogVideoXTransformer3DModelTraj.enable_mxfp8):
//   orv_mxfp8_quantize : bf16 [M, K] -> e4m3fn q [M, K] + e8m0 scales [M, K / 32] (the format: mxfp8.hpp)
//   orv_gemm_mxfp8     : C = epilogue(A . W^T + bias), A and W in MXFP8, fp32 accumulation, bf16 C
//
// The GEMM is gemm_kernel's structure (gemm.hip) on the block-scaled MFMA v_mfma_scale_f32_32x32x64_f8f6f4 (e4m3 x e4m3, twice the
// bf16 MFMA rate per clock): 8 waves in 4 (M) x 2 (N), BM x BN tile, one K-tile = 128 elements = one 128-byte line per row (the same
// staging geometry as the bf16 kernel's 64-element K-tile), global_load_lds into a double-buffered, source-swizzled LDS image, one
// barrier per K-tile, two MFMA k-steps of 64 per K-tile.  The e8m0 scales go straight into the MFMA's scale operands.
//
// Lane map of the scaled MFMA (measured with exact-integer operands and per-lane scales, profiles/mxfp8_lane_map.txt): lane l holds
// row (l & 31) of its operand; bytes 0-15 of its 32 are elements 16 (l >> 5) + [0, 16) of the step's FIRST 32-element block,
// bytes 16-31 the same positions of the SECOND block; its scale operand (byte 0) is the scale of block (l >> 5) of its row.  So a lane
// reads 16-byte chunks (4 ks + h) and (4 ks + 2 + h) of its row's 128-byte K-tile line (h = l >> 5) and takes scale byte 2 ks + h of
// the K-tile.  The accumulator layout is the bf16 32x32 one, so with the W fragment as the MFMA's A operand it holds C^T exactly like
// gemm_kernel's and gemm_epilogue (gemm_epilogue.hpp) stores it unchanged.
//
// No split-K and a tile that depends on N only: every output element is one fixed chain of MFMAs over K, whatever M.
#include "gemm_epilogue.hpp"
#include "mxfp8.hpp"

namespace {

typedef __attribute__((ext_vector_type(8))) int i32x8;

// one lane per 16-byte chunk; lanes past the end compute the last chunk again and do not store
__global__ __launch_bounds__(256) void mxfp8_quantize_kernel(const bf16_t* __restrict__ x, long ldx, uint8_t* __restrict__ q,
                                                             uint8_t* __restrict__ s, int M, int K) {
    const int kc = K >> 3;
    const long nch = (long)M * kc;
    const long t0 = (long)blockIdx.x * 256 + threadIdx.x;
    const long t = t0 < nch ? t0 : nch - 1;
    const long row = t / kc;
    const int c = (int)(t - row * kc);
    const uint4 v = *(const uint4*)(x + row * ldx + (long)c * 8);
    uint2 qq;
    uint32_t sb;
    mx_quantize8(v, qq, sb);
    if (t0 < nch) mx_store8(q + row * K, s + row * (K >> 5), c, qq, sb);
}

template <int BM, int BN, int EPI>
__global__ __launch_bounds__(512) void gemm_mxfp8_kernel(const GemmArgs p, const uint8_t* __restrict__ sa, const uint8_t* __restrict__ sw) {
    constexpr int WM = 4, WN = 2;
    constexpr int MB = BM / (32 * WM);   // 32-row blocks per wave along M
    constexpr int NB = BN / (32 * WN);   // 32-col blocks per wave along N
    static_assert(BM % (32 * WM) == 0 && BN % (32 * WN) == 0 && BM % 64 == 0 && BN % 64 == 0, "tile / wave grid mismatch");
    constexpr int A_BYTES = BM * 128;    // one stage of A: BM rows x 128 e4m3
    constexpr int B_BYTES = BN * 128;
    constexpr int STAGE = A_BYTES + B_BYTES;
    constexpr int A_LD = BM / 64;        // glds pieces per wave per stage (each moves 8 rows)
    constexpr int B_LD = BN / 64;
    constexpr int NP = A_LD + B_LD;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const uint8_t* A = (const uint8_t*)p.A;
    const uint8_t* W = (const uint8_t*)p.W;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int tm, tn;
    tile_of_block(p, tm, tn);
    const int m0 = tm * BM, n0 = tn * BN;

    // staging sources, swizzled on the SOURCE side: 16-byte chunk c of tile row r sits in slot c ^ ((r >> 1) & 7)
    const uint8_t* a_src[A_LD];
    const uint8_t* b_src[B_LD];
    const int srow = lane >> 3, slot = lane & 7;
#pragma unroll
    for (int j = 0; j < A_LD; ++j) {
        const int row = (wave * A_LD + j) * 8 + srow;
        a_src[j] = A + (long)min(m0 + row, p.M - 1) * p.lda + (slot ^ ((row >> 1) & 7)) * 16;
    }
#pragma unroll
    for (int j = 0; j < B_LD; ++j) {
        const int row = (wave * B_LD + j) * 8 + srow;
        b_src[j] = W + (long)(n0 + row) * p.ldw + (slot ^ ((row >> 1) & 7)) * 16;
    }
    auto issue_piece = [&](int pc, int s, long koff) {
        if (pc < A_LD) glds16(a_src[pc] + koff, smem + s * STAGE + (wave * A_LD + pc) * 1024);
        else glds16(b_src[pc - A_LD] + koff, smem + s * STAGE + A_BYTES + (wave * B_LD + (pc - A_LD)) * 1024);
    };

    const int wm = wave / WN, wn = wave % WN;
    const int l31 = lane & 31, hi = lane >> 5, sw8 = (lane >> 1) & 7;
    const int a_row_off = (wm * (BM / WM) + l31) * 128;
    const int b_row_off = A_BYTES + (wn * (BN / WN) + l31) * 128;
    // scale rows of this lane: 4 bytes (the 4 blocks of one K-tile) per row and K-tile
    const int kb = p.K >> 5;
    const uint32_t* sa_row[MB];
    const uint32_t* sw_row[NB];
#pragma unroll
    for (int j = 0; j < MB; ++j) sa_row[j] = (const uint32_t*)(sa + (long)min(m0 + wm * (BM / WM) + j * 32 + l31, p.M - 1) * kb);
#pragma unroll
    for (int i = 0; i < NB; ++i) sw_row[i] = (const uint32_t*)(sw + (long)(n0 + wn * (BN / WN) + i * 32 + l31) * kb);

    f32x16 acc[NB][MB];
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int j = 0; j < MB; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    auto read_frag = [&](const char* base, int ks) {
        const uint4 lo = *(const uint4*)(base + (((ks * 4 + hi) ^ sw8) * 16));
        const uint4 up = *(const uint4*)(base + (((ks * 4 + 2 + hi) ^ sw8) * 16));
        i32x8 f;
        f[0] = lo.x; f[1] = lo.y; f[2] = lo.z; f[3] = lo.w; f[4] = up.x; f[5] = up.y; f[6] = up.z; f[7] = up.w;
        return f;
    };

    const int nk = p.K / 128;
    uint32_t sa_cur[MB], sw_cur[NB];
#pragma unroll
    for (int j = 0; j < MB; ++j) sa_cur[j] = sa_row[j][0];
#pragma unroll
    for (int i = 0; i < NB; ++i) sw_cur[i] = sw_row[i][0];
#pragma unroll
    for (int pc = 0; pc < NP; ++pc) issue_piece(pc, 0, 0);
    int cs = 0;
    for (int t = 0; t < nk; ++t) {
        // tile t has landed for this wave; after the barrier for all waves, and nobody still reads the other stage
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        const char* sbase = smem + cs * STAGE;
        const int tn1 = t + 1 < nk ? t + 1 : 0;              // the last iteration re-fetches tile 0 (never read)
        const long koff = (long)tn1 * 128;
        uint32_t sa_nxt[MB], sw_nxt[NB];
#pragma unroll
        for (int j = 0; j < MB; ++j) sa_nxt[j] = sa_row[j][tn1];
#pragma unroll
        for (int i = 0; i < NB; ++i) sw_nxt[i] = sw_row[i][tn1];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            i32x8 af[MB], bf[NB];
            int sak[MB], swk[NB];
            const int sh = 8 * (2 * ks + hi);
#pragma unroll
            for (int j = 0; j < MB; ++j) { af[j] = read_frag(sbase + a_row_off + j * 32 * 128, ks); sak[j] = (sa_cur[j] >> sh) & 0xff; }
#pragma unroll
            for (int i = 0; i < NB; ++i) { bf[i] = read_frag(sbase + b_row_off + i * 32 * 128, ks); swk[i] = (sw_cur[i] >> sh) & 0xff; }
#pragma unroll
            for (int pc = 0; pc < NP; ++pc)
                if (pc * 2 / NP == ks) issue_piece(pc, cs ^ 1, koff);
#pragma unroll
            for (int i = 0; i < NB; ++i)
#pragma unroll
                for (int j = 0; j < MB; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(bf[i], af[j], acc[i][j], 0, 0, 0, swk[i], 0, sak[j]);
        }
#pragma unroll
        for (int j = 0; j < MB; ++j) sa_cur[j] = sa_nxt[j];
#pragma unroll
        for (int i = 0; i < NB; ++i) sw_cur[i] = sw_nxt[i];
        cs ^= 1;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

    gemm_epilogue<NB, MB, EPI>(p, acc, m0 + wm * (BM / WM), n0 + wn * (BN / WN), lane);
}

template <int BM, int BN, int EPI>
int launch_mxfp8(const GemmArgs& a, const uint8_t* sa, const uint8_t* sw, hipStream_t st) {
    constexpr int smem = 2 * (BM + BN) * 128;
    static bool attr_done = false;
    if (!attr_done) {
        (void)hipFuncSetAttribute((const void*)gemm_mxfp8_kernel<BM, BN, EPI>, hipFuncAttributeMaxDynamicSharedMemorySize, smem);
        attr_done = true;
    }
    hipLaunchKernelGGL((gemm_mxfp8_kernel<BM, BN, EPI>), dim3(a.tiles_m * a.tiles_n), dim3(512), smem, st, a, sa, sw);
    return orv_check_launch("orv_gemm_mxfp8");
}

template <int BN>
int dispatch_mxfp8(const GemmArgs& a, int epi, const uint8_t* sa, const uint8_t* sw, hipStream_t st) {
    switch (epi) {
        case 0: return launch_mxfp8<256, BN, 0>(a, sa, sw, st);
        case 1: return launch_mxfp8<256, BN, 1>(a, sa, sw, st);
        case 2: return launch_mxfp8<256, BN, 2>(a, sa, sw, st);
        default: orv_set_error("orv_gemm_mxfp8: epilogue %d (0, 1 or 2)", epi); return ORV_EINVAL;
    }
}

}  // namespace

extern "C" int orv_mxfp8_quantize(const void* x, long ldx, void* q, void* s, int M, int K, void* stream) {
    ORV_REQUIRE(x && q && s, "orv_mxfp8_quantize: null operand");
    ORV_REQUIRE(M > 0 && K > 0 && K % 32 == 0, "orv_mxfp8_quantize: M=%d K=%d (K %% 32 == 0)", M, K);
    ORV_REQUIRE(ldx >= K && ldx % 8 == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)q & 7) == 0,
                "orv_mxfp8_quantize: x needs 16-byte aligned rows (ldx %% 8 == 0, ldx >= K), q 8-byte alignment");
    const long nch = (long)M * (K / 8);
    hipLaunchKernelGGL(mxfp8_quantize_kernel, dim3((unsigned)((nch + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)x, ldx, (uint8_t*)q, (uint8_t*)s, M, K);
    return orv_check_launch("orv_mxfp8_quantize");
}

extern "C" int orv_gemm_mxfp8(const orv_gemm_t* g, const void* a_scale, const void* w_scale, void* stream) {
    ORV_REQUIRE(g && g->A && g->W && g->C && a_scale && w_scale, "orv_gemm_mxfp8: null operand");
    ORV_REQUIRE(g->M > 0 && g->N > 0 && g->K > 0, "orv_gemm_mxfp8: empty problem M=%d N=%d K=%d", g->M, g->N, g->K);
    ORV_REQUIRE(g->K % 128 == 0, "orv_gemm_mxfp8: K=%d must be a multiple of 128", g->K);
    ORV_REQUIRE(g->N % 128 == 0, "orv_gemm_mxfp8: N=%d must be a multiple of 128", g->N);
    ORV_REQUIRE(g->epilogue >= 0 && g->epilogue <= 2, "orv_gemm_mxfp8: epilogue %d (0, 1 or 2)", g->epilogue);
    ORV_REQUIRE(g->lda >= g->K && g->ldw >= g->K && g->lda % 16 == 0 && g->ldw % 16 == 0 && ((uintptr_t)g->A & 15) == 0 &&
                    ((uintptr_t)g->W & 15) == 0 && ((uintptr_t)a_scale & 3) == 0 && ((uintptr_t)w_scale & 3) == 0,
                "orv_gemm_mxfp8: A / W need 16-byte aligned rows (lda, ldw multiples of 16), scales 4-byte alignment");
    ORV_REQUIRE(g->ldc % 8 == 0 && ((uintptr_t)g->C & 15) == 0 && (!g->R || (((uintptr_t)g->R & 15) == 0 && g->ldr % 8 == 0)),
                "orv_gemm_mxfp8: C / R must be 16-byte aligned with leading dimensions that are multiples of 8");
    ORV_REQUIRE(g->epilogue != 2 || g->R, "orv_gemm_mxfp8: epilogue 2 needs R");
    ORV_REQUIRE(g->epilogue != 2 || !g->gate || g->grp.seq > 0, "orv_gemm_mxfp8: gate needs grp.seq");
    ORV_REQUIRE(!g->Y && !g->a_packed && !g->c_packed, "orv_gemm_mxfp8: no Y output and no packed operands (inference only)");
    GemmArgs a{};   // no Y / packing / walk-back / grid knobs
    a.A = (const bf16_t*)g->A; a.lda = g->lda; a.W = (const bf16_t*)g->W; a.ldw = g->ldw;   // byte rows (e4m3)
    a.bias = (const bf16_t*)g->bias; a.C = (bf16_t*)g->C; a.ldc = g->ldc;
    a.M = g->M; a.N = g->N; a.K = g->K;
    a.R = (const bf16_t*)g->R; a.ldr = g->ldr; a.r_mod = g->r_mod;
    a.gate = g->gate; a.gate_b = g->gate_b; a.gate_g = g->gate_g;
    a.seq = g->grp.seq; a.n_text = g->grp.n_text; a.per_group = g->grp.per_group;
    a.c_rows = g->cmap.rows; a.c_bstride = g->cmap.bstride; a.c_off = g->cmap.off;
    // tile from N alone: 256 x 256 where N allows, else 256 x 128
    const int bn = g->N % 256 == 0 ? 256 : 128;
    a.tiles_m = (g->M + 255) / 256;
    a.tiles_n = g->N / bn;
    hipStream_t st = (hipStream_t)stream;
    const uint8_t *sa = (const uint8_t*)a_scale, *sw = (const uint8_t*)w_scale;
    return bn == 256 ? dispatch_mxfp8<256>(a, g->epilogue, sa, sw, st) : dispatch_mxfp8<128>(a, g->epilogue, sa, sw, st);
}
