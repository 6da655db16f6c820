// bf16 GEMM  C = epilogue(A[M,K] . W[N,K]^T + bias), the "d8" kernel (round 5): the 256-row tile of gemm_t8_kernel with MORE BYTES IN
// FLIGHT.  Round 4 measured the t8 K loop (profiles/r4_gemm_t8_load_side.txt): its LDS-DMA stream alone takes as long as its MFMA stream
// because it is latency x bytes-in-flight bound - two 64-KB K-tile buffers fill the 160 KB of LDS, so at most ~48 KB per CU are in flight
// against ~1 us of L2-miss latency.  Here only ONE operand goes through LDS:
//   * 8 waves as 8 (M) x 1 (N): a wave owns 32 rows x BN columns (2 x BN/16 accumulator blocks of v_mfma_f32_16x16x32_bf16, C^T form as t8).
//   * A: each wave loads ITS OWN 32 rows x 64 k of every K-tile straight into the MFMA B-operand layout (4 x global_load_dwordx4), TWO
//     K-tiles ahead, into a ring of three register sets (48 VGPRs).  No wave shares A rows with another, so nothing is fetched twice and
//     nothing is staged.  The operand layout (lane = row l & 15, 16-byte k chunk l >> 4) puts the four lanes of a quad into four different
//     rows: read from a ROW-MAJOR A that shape moves 18.8 B/clk/CU through the texture path against 62 for quad- or line-contiguous
//     instructions (tools/probe_frag_loads.cpp, profiles/r5_probe_frag_loads.txt) and the first d8 build lost 10-17 % to t8 because of it
//     (profiles/r5_gemm_d8.txt).  So A must be in the PACKED layout "P16" (include/orv_mi355.h, orv_gemm_t.a_packed): 1-KiB blocks of 16 rows
//     x 32 k stored in exactly the order a wave instruction wants them (lane l's 16 bytes at l * 16) - every load is one contiguous KiB.
//     A's producers write that layout directly: an MFMA kernel's accumulator layout has lane = row, so its epilogue stores a packed
//     block as one lane-linear 1-KiB instruction (c_packed below: cheaper than the row-major store), orv_layernorm_modulate scatters.
//   * W: BN rows x 64 k per K-tile by LDS-DMA in full-line pieces (8 rows x 128 B, chunk ^ (row & 6): t8's round-4 image), FOUR buffers
//     of BN x 128 B, filled THREE K-tiles ahead and waited for ONE K-tile early.  Every wave reads every W fragment (ds_read_b128).
//   -> ~2 x (32 + 32) KB in flight per CU instead of ~48, LDS-DMA instructions halved (4 + 4 plain loads per wave and K-tile instead of 8
//      DMA), ONE s_barrier per K-tile instead of eight (a buffer is known complete a whole K-tile before it is read, so fragment reads
//      run ahead across K-tile boundaries), no ping-pong choreography: the two waves of a SIMD free-run and fill each other's gaps.
//   Costs: 256 KB (BN = 256) of fragment reads per K-tile and CU instead of 192 (1024 of 2048 LDS cycles), a W fragment feeds 2 MFMAs.
//   * persistent over the XCD-aware tile list, both streams keep their own (tile, K-tile) cursor and run on into the next tile under the
//     epilogue, like t8.
//   * epilogues 0-4 through the per-wave LDS transpose (t8_epilogue_lds's arithmetic, element for element): a wave owns whole rows of the
//     tile, 64 columns at a time = one head for the fused qk LayerNorm.  The accumulation order per output element is t8's (K-tiles
//     ascending, k halves 0, 1, the same k chunk per lane group), so the results are bit-identical to gemm_t8_kernel's.
// Requires a_packed, K % 192 == 0 (three register sets, statically indexed: the K loop is unrolled by three), N % BN == 0, W < 4 GiB.
#include "gemm_common.hpp"
#include <type_traits>

namespace {
using namespace orv_gemm;

__device__ __forceinline__ void d8_unpack8(const uint4 u, float (&f)[8]) {
    f[0] = bf2f(u.x & 0xffff); f[1] = bf2f(u.x >> 16); f[2] = bf2f(u.y & 0xffff); f[3] = bf2f(u.y >> 16);
    f[4] = bf2f(u.z & 0xffff); f[5] = bf2f(u.z >> 16); f[6] = bf2f(u.w & 0xffff); f[7] = bf2f(u.w >> 16);
}
__device__ __forceinline__ uint4 d8_pack8(const float (&f)[8]) {
    return make_uint4(pack2bf(f[0], f[1]), pack2bf(f[2], f[3]), pack2bf(f[4], f[5]), pack2bf(f[6], f[7]));
}
__device__ __forceinline__ float d8_sum_quad(float v) {      // (v(l) + v(l ^ 1)) + (v(l ^ 2) + v(l ^ 3)) in every lane of a quad
    v += __uint_as_float(__builtin_amdgcn_update_dpp(0, __float_as_uint(v), 0xB1, 0xF, 0xF, true));     // quad_perm [1,0,3,2]
    v += __uint_as_float(__builtin_amdgcn_update_dpp(0, __float_as_uint(v), 0x4E, 0xF, 0xF, true));     // quad_perm [2,3,0,1]
    return v;
}
__device__ __forceinline__ float d8_shl4(float v) {          // v(lane + 4) within a row of 16 lanes (row_shl:4)
    return __uint_as_float(__builtin_amdgcn_update_dpp(0, __float_as_uint(v), 0x104, 0xF, 0xF, true));
}
__device__ __forceinline__ float d8_shr4(float v) {          // v(lane - 4) within a row of 16 lanes (row_shr:4)
    return __uint_as_float(__builtin_amdgcn_update_dpp(0, __float_as_uint(v), 0x114, 0xF, 0xF, true));
}
__device__ __forceinline__ unsigned long long d8_uniform64(unsigned long long u) {
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)u), hi = __builtin_amdgcn_readfirstlane((unsigned)(u >> 32));
    return ((unsigned long long)hi << 32) | lo;
}

// Epilogue of one wave: rows row0 .. row0 + 31 (two 16-row blocks), columns col0 .. col0 + BN - 1 in groups of 64.  Accumulator layout
// (as t8): lane (r16 = lane & 15, g = lane >> 4) holds, of block 2 P + t of a 64-column group, columns 32 P + 8 g + 4 t + (0..3) of row r16.
// Every (16 rows x 64 columns) piece goes through the wave's 4-KiB fp32 scratch and comes back as lane = (row lane >> 3, 8-column chunk
// lane & 7): loads and stores are 8 rows x one full 128-byte line per instruction.
// Row-operand epilogues (2 = gated residual, 3 = GELU adjoint).  Up to round 6 the rows of a 64-column group were requested when the group
// started, the bias behind them and the gate values inside the row-block loop, each used at once: every one of those loads sat BEHIND the
// previous stores, and since the vector-memory counter retires in order, waiting for it meant waiting for those stores' acknowledgements too -
// 41 full drains in gemm_d8_kernel<192, 2> against 10 in the plain kernel.  A second residual register set (round 5) and residual rows
// staged by LDS-DMA only moved the residual rows and left that chain in place, which is why both measured level.  Now d8_epilogue gathers bias and
// gate before the tile's first store and rolls ONE residual set a group ahead (profiles/r7_gemm_gated_epilogue.txt).

template <int BN, int EPI, int RB = 2>
__device__ __forceinline__ void d8_epilogue(const GemmArgs& p, f32x4 (&acc)[RB][BN / 16], const int row0, const int col0, const int lane,
                                            char* const scr) {
    constexpr int NG = BN / 64;
    const int g = lane >> 4, r16 = lane & 15;
    const int c = lane & 7, rr8 = lane >> 3;
    int woff[4];
#pragma unroll
    for (int blk = 0; blk < 4; ++blk) {
        const int L = 8 * (blk >> 1) + 2 * g + (blk & 1);
        woff[blk] = r16 * 256 + ((L ^ (r16 & 7)) << 4);
    }
    const int roff0 = rr8 * 256 + (((2 * c) ^ rr8) << 4), roff1 = rr8 * 256 + (((2 * c + 1) ^ rr8) << 4);      // + j * 2048

    constexpr bool GATH = EPI == 2 || EPI == 3;
    // output row numbers: 32 bits in the row-operand epilogues at BN = 256, which have no register to spare (launch_d8 checks the range)
    using row_t = std::conditional_t<GATH && BN == 256, int, long>;
    row_t orow[RB][2];
    bool valid[RB][2];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int m = row0 + rb * 16 + 8 * j + rr8;
            valid[rb][j] = m < p.M;
            const int mc = min(m, p.M - 1);
            orow[rb][j] = mc;
            if (p.c_rows > 0) orow[rb][j] = (row_t)((long)(mc / p.c_rows) * p.c_bstride + p.c_off + mc % p.c_rows);
        }
    // gate rows (EPI 2) of the wave's rows, found once per tile (integer divisions on the scalar unit).  Token groups are 226 / 600 rows long,
    // so the 16 RB rows of a wave lie inside one (batch element, token group) or cross one boundary: gseg = 1: every row takes the gate row
    // of the wave's first row (A); 2: A or the gate row of the wave's last row (B), in_a[rb][j] says which for this lane's row; 3: more
    // than two gate rows (groups shorter than the wave's rows) - only then are the gate values loaded per lane in the loop.
    const float *gate_a = nullptr, *gate_b = nullptr;
    int gseg = 0;
    bool in_a[RB][2];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) in_a[rb][0] = in_a[rb][1] = true;
    if (EPI == 2 && p.gate) {
        const int mf = __builtin_amdgcn_readfirstlane(row0);
        long of = min(mf, p.M - 1), ol = min(mf + 16 * RB - 1, p.M - 1);
        if (p.c_rows > 0) {
            of = (long)(of / p.c_rows) * p.c_bstride + p.c_off + of % p.c_rows;
            ol = (long)(ol / p.c_rows) * p.c_bstride + p.c_off + ol % p.c_rows;
        }
        const int bf_ = (int)(of / p.seq), bl_ = (int)(ol / p.seq);
        const int gf_ = orv_group_of((int)(of % p.seq), p.n_text, p.per_group);
        const int gl_ = orv_group_of((int)(ol % p.seq), p.n_text, p.per_group);
        gate_a = p.gate + bf_ * p.gate_b + gf_ * p.gate_g;
        gseg = 1;
        if (bf_ != bl_ || gf_ != gl_) {
            gate_b = p.gate + bl_ * p.gate_b + gl_ * p.gate_g;
            // rows ascend from the first to the last row of the wave (the uniform test above relies on the same): a row is in A below the end
            // of A's (batch element, token group), in B from the start of B's - no division per lane
            const int ea_ = gf_ == 0 ? p.n_text : (p.per_group > 0 ? p.n_text + gf_ * p.per_group : p.seq);
            const long end_a = (long)bf_ * p.seq + min(ea_, p.seq);
            const long start_b = (long)bl_ * p.seq + (gl_ == 0 ? 0 : p.n_text + (gl_ - 1) * max(p.per_group, 0));
            bool other = false;
#pragma unroll
            for (int rb = 0; rb < RB; ++rb)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    in_a[rb][j] = orow[rb][j] < end_a;
                    other = other || !(in_a[rb][j] || orow[rb][j] >= start_b);
                }
            gseg = (BN == 256 || __builtin_amdgcn_ballot_w64(other) != 0) ? 3 : 2;       // BN = 256 has no registers for row B: per lane as well
        }
    }
    // row operands (residual / GELU-adjoint input): ONE register set, rolling.  Group 0's rows are requested up front; the piece (rb, j) of
    // group cg + 1 is requested into the registers of piece (rb, j) of group cg as soon as that one has been read, i.e. IN FRONT of the
    // piece's own store and a whole group before it is used.  These loads are unconditional, so every wait of the loop is a counted one: it
    // leaves the youngest stores in flight (d8_epilogue's note on the gather below; profiles/r7_gemm_gated_epilogue.txt).
    uint4 r8[RB][2];                                    // [rb][j]
    auto load_row = [&](int cg, int rb, int j) {
        long rr = orow[rb][j];                          // the output row (row map included) unless the residual is a table
        if (p.r_mod > 0) rr = min(row0 + rb * 16 + 8 * j + rr8, p.M - 1) % p.r_mod;
        return *(const uint4*)(p.R + rr * p.ldr + col0 + 64 * cg + 8 * c);
    };
    if (GATH) {
#pragma unroll
        for (int rb = 0; rb < RB; ++rb)
#pragma unroll
            for (int j = 0; j < 2; ++j) r8[rb][j] = load_row(0, rb, j);
    }
    // Gather (row-operand epilogues): every bias and gate value of the tile is requested HERE, before the tile's first store, in "source
    // layout" - lane l holds column 64 cg + l, ONE register per (64-column group, row) - and handed to the lanes that need it (lane (row
    // lane >> 3, chunk c) wants columns 8 c .. 8 c + 7) by ds_bpermute in the loop.  The vector-memory counter retires in order: a load issued
    // behind a store can only be waited for together with that store's acknowledgement, and the old form (bias per group, gate values per row
    // block, each used at once) was a chain of ~30 such round trips per tile and wave.
    const int bp = c << 5;                              // ds_bpermute byte address of lane 8 c
    uint32_t bsrc[NG];
    float gsrc_a[NG], gsrc_b[NG];                       // gate rows A and B
#pragma unroll
    for (int cg = 0; cg < NG; ++cg) { bsrc[cg] = 0; gsrc_a[cg] = gsrc_b[cg] = 1.f; }
    if constexpr (GATH) {
        if (p.bias) {
#pragma unroll
            for (int cg = 0; cg < NG; ++cg) bsrc[cg] = p.bias[col0 + 64 * cg + lane];
        }
        if (gseg == 1 || gseg == 2) {
#pragma unroll
            for (int cg = 0; cg < NG; ++cg) gsrc_a[cg] = gate_a[col0 + 64 * cg + lane];
        }
        if (gseg == 2) {
#pragma unroll
            for (int cg = 0; cg < NG; ++cg) gsrc_b[cg] = gate_b[col0 + 64 * cg + lane];
        }
    }
    // out[e] = src of lane 8 c + e.  Inline asm for the instruction's offset field: the builtin keeps eight address registers alive instead.
    auto spread8 = [&](uint32_t src, uint32_t (&o)[8]) {
        asm volatile("ds_bpermute_b32 %0, %8, %9\n\tds_bpermute_b32 %1, %8, %9 offset:4\n\tds_bpermute_b32 %2, %8, %9 offset:8\n\t"
                     "ds_bpermute_b32 %3, %8, %9 offset:12\n\tds_bpermute_b32 %4, %8, %9 offset:16\n\tds_bpermute_b32 %5, %8, %9 offset:20\n\t"
                     "ds_bpermute_b32 %6, %8, %9 offset:24\n\tds_bpermute_b32 %7, %8, %9 offset:28\n\ts_waitcnt lgkmcnt(0)"
                     : "=&v"(o[0]), "=&v"(o[1]), "=&v"(o[2]), "=&v"(o[3]), "=&v"(o[4]), "=&v"(o[5]), "=&v"(o[6]), "=&v"(o[7])
                     : "v"(bp), "v"(src));
    };

#pragma unroll
    for (int cg = 0; cg < NG; ++cg) {
        const int col8 = col0 + 64 * cg + 8 * c;
        float b8[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) b8[e] = 0.f;
        if (p.bias) {
            if constexpr (GATH) {
                uint32_t o[8];
                spread8(bsrc[cg], o);
#pragma unroll
                for (int e = 0; e < 8; ++e) b8[e] = bf2f((bf16_t)o[e]);
            } else {
                d8_unpack8(*(const uint4*)(p.bias + col8), b8);
            }
        }
        // epilogue 4: qk LayerNorm parameters of this lane's 8 channels of the head (the 64-column group IS one head)
        float ga[8], be[8];
        int region = 2;
        float post = 1.f;
        if constexpr (EPI == 4) {
            region = __builtin_amdgcn_readfirstlane((col0 + 64 * cg) / (p.qn_heads * 64));     // 0 = q, 1 = k, 2 = v
            const bf16_t* gam = region == 0 ? p.qn_gq : p.qn_gk;
            const bf16_t* bet = region == 0 ? p.qn_bq : p.qn_bk;
            post = region == 0 ? p.qn_premul : 1.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) { ga[e] = 1.f; be[e] = 0.f; }
            if (region < 2 && gam) d8_unpack8(*(const uint4*)(gam + 8 * c), ga);
            if (region < 2 && bet) d8_unpack8(*(const uint4*)(bet + 8 * c), be);
        }
        float g8[8];                                     // gate row A, this lane's 8 columns of the group
#pragma unroll
        for (int e = 0; e < 8; ++e) g8[e] = 1.f;
        if (gseg == 1 || gseg == 2) {
            uint32_t o[8];
            spread8(__float_as_uint(gsrc_a[cg]), o);
#pragma unroll
            for (int e = 0; e < 8; ++e) g8[e] = __uint_as_float(o[e]);
        }

#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
#pragma unroll
            for (int blk = 0; blk < 4; ++blk) *(f32x4*)(scr + woff[blk]) = acc[rb][4 * cg + blk];
            float v[2][8];
            auto read_v = [&](int j) {
                const f32x4 lo = *(const f32x4*)(scr + j * 2048 + roff0), hi = *(const f32x4*)(scr + j * 2048 + roff1);
                v[j][0] = lo[0]; v[j][1] = lo[1]; v[j][2] = lo[2]; v[j][3] = lo[3];
                v[j][4] = hi[0]; v[j][5] = hi[1]; v[j][6] = hi[2]; v[j][7] = hi[3];
            };
            if constexpr (!GATH) { read_v(0); read_v(1); }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                if constexpr (GATH) {       // one row at a time (8 registers less at the point where everything else is alive)
                    asm volatile("" ::: "memory");
                    read_v(j);
                }
                float (&w)[8] = v[j];
                uint4 rcur;
                if constexpr (GATH) {
                    rcur = r8[rb][j];
                    if (cg + 1 < NG) r8[rb][j] = load_row(cg + 1, rb, j);
                }
#pragma unroll
                for (int e = 0; e < 8; ++e) w[e] += b8[e];
                bf16_t* crow = p.C + orow[rb][j] * p.ldc + col8;
                if (p.Y && valid[rb][j]) *(uint4*)(p.Y + orow[rb][j] * p.ldy + col8) = d8_pack8(w);
                if constexpr (EPI == 4) {
                    if (region < 2) {
                        // The statistics are summed in gemm_t8_kernel's ORDER, so that the two kernels agree bit for bit here as well (a one-clip call takes
                        // this kernel for q | k | v, a four-clip call the t8 pair: B = 4 stays bit-identical to four B = 1 calls).  t8's lane g of a row holds
                        // columns 8 g .. 8 g + 7 and 32 + 8 g .. + 7 and chains its 16 values in that order, then adds lane g ^ 1, then g ^ 2.  Here lane c
                        // holds chunk c: lanes c < 4 fetch chunk c + 4 of their row (row_shl:4), chain like t8's lane g = c, combine inside the quad, and
                        // hand the result to lanes c >= 4 (row_shr:4).
                        float hi[8];
#pragma unroll
                        for (int e = 0; e < 8; ++e) hi[e] = d8_shl4(w[e]);
                        float s = 0.f;
#pragma unroll
                        for (int e = 0; e < 8; ++e) s += w[e];
#pragma unroll
                        for (int e = 0; e < 8; ++e) s += hi[e];
                        s = d8_sum_quad(s);
                        const float s_up = d8_shr4(s);       // every lane executes the cross-lane moves (a DPP inside a divergent arm reads disabled lanes)
                        const float mean = (c < 4 ? s : s_up) * (1.f / 64.f);
                        float sq = 0.f;
#pragma unroll
                        for (int e = 0; e < 8; ++e) { w[e] -= mean; sq = qkln_sq(w[e], sq); }
#pragma unroll
                        for (int e = 0; e < 8; ++e) { hi[e] -= mean; sq = qkln_sq(hi[e], sq); }
                        sq = d8_sum_quad(sq);
                        const float sq_up = d8_shr4(sq);
                        const float rstd = rsqrtf((c < 4 ? sq : sq_up) * (1.f / 64.f) + p.qn_eps);
#pragma unroll
                        for (int e = 0; e < 8; ++e) w[e] = qkln_affine(w[e], rstd, ga[e], be[e], post);
                    }
                }
                if (EPI == 1) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) w[e] = gelu_tanh(w[e]);
                }
                if (EPI == 2) {
                    float rv[8], gg[8];
                    d8_unpack8(rcur, rv);
#pragma unroll
                    for (int e = 0; e < 8; ++e) gg[e] = g8[e];
                    if (gseg == 2) {         // the wave crosses one group boundary: this lane's row takes gate row A or B
                        uint32_t o[8];
                        spread8(__float_as_uint(gsrc_b[cg]), o);
#pragma unroll
                        for (int e = 0; e < 8; ++e) gg[e] = in_a[rb][j] ? g8[e] : __uint_as_float(o[e]);
                    }
                    // more gate rows than the gather holds: this lane's rows pick their own.  Both rows of the block are loaded here (one wait
                    // per block, on this path only); row 1's values wait in g8, which this path does not use otherwise
                    if (gseg == 3 && j == 0) {
                        f32x4 q[2][2];
#pragma unroll
                        for (int jj = 0; jj < 2; ++jj) {
                            const unsigned o_ = (unsigned)orow[rb][jj];          // below 2^31: launch_d8 checks (a 32-bit division per lane)
                            const int bidx = (int)(o_ / (unsigned)p.seq), sq_ = (int)(o_ - (unsigned)bidx * (unsigned)p.seq);
                            const float* grow = p.gate + bidx * p.gate_b + orv_group_of(sq_, p.n_text, p.per_group) * p.gate_g;
                            q[jj][0] = *(const f32x4*)(grow + col8);
                            q[jj][1] = *(const f32x4*)(grow + col8 + 4);
                        }
                        asm volatile("" : "+v"(q[0][0]), "+v"(q[0][1]), "+v"(q[1][0]), "+v"(q[1][1]));
#pragma unroll
                        for (int e = 0; e < 8; ++e) { gg[e] = q[0][e >> 2][e & 3]; g8[e] = q[1][e >> 2][e & 3]; }
                    }
#pragma unroll
                    for (int e = 0; e < 8; ++e) w[e] = rv[e] + gg[e] * w[e];
                }
                if (EPI == 3) {
                    float rv[8];
                    d8_unpack8(rcur, rv);
#pragma unroll
                    for (int e = 0; e < 8; ++e) w[e] *= gelu_tanh_grad(rv[e]);
                }
                if (valid[rb][j]) *(uint4*)crow = d8_pack8(w);
            }
        }
    }
}

// Packed output (c_packed, epilogues 0 / 1): C in the P16 layout of an [M, N] matrix, i.e. ready to be the NEXT GEMM's A operand (FFN1 -> FFN2:
// cogvideox_control.py:439-440).  In the accumulator layout lane (r16, g) holds columns 32 P + 8 g + (0..7) of row r16 for the block pair P -
// that IS packed block (row block, column block col0 / 32 + P) at byte 16 (r16 + 16 g) = 16 lane: one lane-linear, fully contiguous 1-KiB
// store per block pair, no LDS transpose, no row mask (the buffer has tiles_m * 256 rows; rows >= M hold finite garbage nobody reads).
template <int BN, int EPI, int RB = 2>
__device__ __forceinline__ void d8_epilogue_packed(const GemmArgs& p, f32x4 (&acc)[RB][BN / 16], const int row0, const int col0, const int lane) {
    const int g = lane >> 4;
    const long nblk = p.ldc / 32;                      // column blocks per row block (ldc = N of the packed matrix)
#pragma unroll
    for (int P = 0; P < BN / 32; ++P) {
        float b8[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) b8[e] = 0.f;
        if (p.bias) d8_unpack8(*(const uint4*)(p.bias + col0 + 32 * P + 8 * g), b8);
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = acc[rb][2 * P + (e >> 2)][e & 3] + b8[e];
            if (EPI == 1) {
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = gelu_tanh(v[e]);
            }
            char* blk = (char*)p.C + (((long)(row0 / 16 + rb) * nblk + (col0 / 32 + P)) << 10);
            *(uint4*)(blk + lane * 16) = d8_pack8(v);
        }
    }
}

// The kernel body for a wave that owns RB 16-row blocks of a BM-row tile.  BM = 256: every wave RB = 2 (rows 32 wave ..).  BM = 192 (round 6,
// gemm_d8r192_kernel): the FIRST wave of every SIMD (waves 0-3) owns two row blocks (rows 32 wave ..), the SECOND (waves 4-7) one (rows 128 +
// 16 (wave - 4) ..) - three row blocks per SIMD instead of four, so a tile costs 3/4 of the matrix time on every SIMD alike.  M = 3226 (one
// clip) is 17 such row tiles: 255 tiles of 192 x 128 (FFN2 / out-projection: ONE full round instead of 195 of 256 CUs busy), 510 of 192 x 192
// for q | k | v (two rounds of 3/4 tiles instead of 1.52 rounds of whole ones).  Both roles run the same W stream, barriers and K loop.
template <int BN, int EPI, int RB, int BM>
__device__ __forceinline__ void d8_body(const GemmArgs& p, char* const smem) {
    static_assert(BM == 256 || BM == 192, "tile rows");
    constexpr int NA = 2 * RB;                        // A loads per wave and K-tile
    constexpr int NCB = BN / 16;                      // 16-column blocks of the tile (16 / 12)
#ifndef ORV_D8_CBP256
#define ORV_D8_CBP256 2
#endif
#ifndef ORV_D8_CBP192
#define ORV_D8_CBP192 3
#endif
    constexpr int CBP = BN == 256 ? ORV_D8_CBP256 : (BN == 192 ? ORV_D8_CBP192 : 2);     // column blocks per phase: BN = 256 eight phases of 8 MFMAs, BN = 192 four of 12, BN = 128 four of 8
    constexpr int NPH = NCB / CBP;
    constexpr int BUFSZ = BN * 128;                   // one K-tile of W: BN rows x 64 k
    constexpr int ND = BN / 64;                       // 1-KiB DMA pieces per wave and K-tile (BN / 8 pieces over 8 waves)
    constexpr int SCR = 4 * BUFSZ;                    // epilogue scratch: 8 waves x 4 KiB behind the four W buffers
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wrb = (BM == 256 || RB == 2) ? 2 * wave : 8 + (wave - 4);      // this wave's first 16-row block inside the tile
    const int ntiles = p.tiles_m * p.tiles_n;
    const int nk = p.K / BK;                          // multiple of 3 (chooser-checked)

    // ---- W stream (LDS-DMA).  Piece q = wave * ND + j: rows 8 (q & 1) .. + 7 of column block q >> 1; lane l fetches row l >> 3, logical
    // 16-byte chunk (l & 7) ^ (row & 6) and lands at physical chunk l & 7 (lane-linear image).  LDS row i of block 2 P + t holds W row
    // 32 P + 8 (i >> 2) + 4 t + (i & 3) of the tile (t8's permutation: a lane's accumulators are 8 contiguous columns per block pair).
    const int dr = lane >> 3;
    const unsigned voffW = (unsigned)(((long)(8 * (dr >> 2) + (dr & 3)) * p.ldw + (((lane & 7) ^ (dr & 6)) << 3)) * 2);
    // Stream cursors wrap WITHOUT a branch (round 6).  The base addresses of the tile a cursor will enter next (wbn / abn) are computed at the
    // top of every compute tile; the wrap inside the K loop is a scalar select.  The old form ran the tile -> address arithmetic (integer
    // divisions) in a rarely taken branch in the middle of the K loop, with A registers in flight from inline-asm loads: the compiler is free
    // to copy live registers on such an edge, and for one instantiation of the refactored kernel it did - it copied load destinations before
    // their data had landed (cdna_hip_programming.md 5.7: an asm load's destination is unprotected until your own wait).
    unsigned long long wb[ND], wbn[ND];               // wave-uniform byte address of the piece's first row at k = 0: cursor's tile / the next one
    int kW = 0, tW = blockIdx.x;
    const unsigned lds0 = (unsigned)(uintptr_t)(const __attribute__((address_space(3))) char*)smem;
#define D8_SETUP_W(DST, TILE)                                                                                        \
    {                                                                                                                \
        int tm_, tn_;                                                                                                \
        tile_of_index(p, min((TILE), ntiles - 1), ntiles, tm_, tn_);                                                 \
        _Pragma("unroll") for (int j = 0; j < ND; ++j) {                                                             \
            const int q_ = wave * ND + j, cb_ = q_ >> 1;                                                             \
            const int wrow_ = tn_ * BN + 32 * (cb_ >> 1) + 16 * (q_ & 1) + 4 * (cb_ & 1);                            \
            DST[j] = d8_uniform64((unsigned long long)(uintptr_t)p.W + (unsigned long long)wrow_ * p.ldw * 2);       \
        }                                                                                                            \
    }
#define D8_WRAP_W()                                                                                                  \
    {                                                                                                                \
        const bool w_ = ++kW == nk;                                                                                  \
        kW = w_ ? 0 : kW;                                                                                            \
        tW += w_ ? (int)gridDim.x : 0;                                                                               \
        _Pragma("unroll") for (int j = 0; j < ND; ++j) wb[j] = w_ ? wbn[j] : wb[j];                                  \
    }
#define D8_DMA1(OFF, SB, LDS) asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" :: "v"(OFF), "s"(SB), "s"(LDS) : "memory", "m0");
#define D8_ISSUE_W(BUFI)                                                                                             \
    {                                                                                                                \
        _Pragma("unroll") for (int j = 0; j < ND; ++j) {                                                             \
            const unsigned long long sb_ = wb[j] + (unsigned long long)kW * 128;                                     \
            const unsigned ld_ = lds0 + (BUFI) * BUFSZ + (wave * ND + j) * 1024;                                     \
            D8_DMA1(voffW, sb_, ld_)                                                                                 \
        }                                                                                                            \
        D8_WRAP_W()                                                                                                  \
    }
    D8_SETUP_W(wb, tW)
    D8_SETUP_W(wbn, tW + (int)gridDim.x)

    // ---- A stream (straight to registers, packed layout).  Block (row block R, k block c) of 16 rows x 32 k sits at ((R * K / 32) + c) KiB;
    // a wave's two row blocks are R = (tile row + 32 wave) / 16 + rb, K-tile kt = blocks 2 kt, 2 kt + 1; lane l takes bytes [16 l, 16 l + 16).
    unsigned voffA[2];
    const unsigned long long rowblk = (unsigned long long)p.K * 32;     // bytes of one 16-row block row
    unsigned long long ab, abn;                                          // wave-uniform byte address of block (R(rb = 0), 0): cursor's tile / the next one
    int kA = 0, tA = blockIdx.x;
    voffA[0] = (unsigned)lane * 16;
    voffA[1] = (unsigned)lane * 16 + (unsigned)rowblk;
#define D8_SETUP_A(DST, TILE)                                                                                        \
    {                                                                                                                \
        int tm_, tn_;                                                                                                \
        tile_of_index(p, min((TILE), ntiles - 1), ntiles, tm_, tn_);                                                 \
        DST = d8_uniform64((unsigned long long)(uintptr_t)p.A + (unsigned long long)(tm_ * (BM / 16) + wrb) * rowblk); \
    }
#define D8_WRAP_A()                                                                                                  \
    {                                                                                                                \
        const bool w_ = ++kA == nk;                                                                                  \
        kA = w_ ? 0 : kA;                                                                                            \
        tA += w_ ? (int)gridDim.x : 0;                                                                               \
        ab = w_ ? abn : ab;                                                                                          \
    }
#define D8_LOADA(DST, OFF, SB, IMM) asm volatile("global_load_dwordx4 %0, %1, %2 offset:" #IMM : "=v"(DST) : "v"(OFF), "s"(SB) : "memory");
#define D8_ISSUE_A(SET)                                                                                              \
    {                                                                                                                \
        const unsigned long long sa_ = ab + (unsigned long long)kA * 2048;                                           \
        D8_LOADA(SET[0], voffA[0], sa_, 0) D8_LOADA(SET[1], voffA[0], sa_, 1024)                                     \
        if constexpr (RB == 2) { D8_LOADA(SET[NA - 2], voffA[1], sa_, 0) D8_LOADA(SET[NA - 1], voffA[1], sa_, 1024) } \
        D8_WRAP_A()                                                                                                  \
    }
    D8_SETUP_A(ab, tA)
    D8_SETUP_A(abn, tA + (int)gridDim.x)

    // ---- W fragment reads: row i = l & 15 of a block = piece i >> 3, row i & 7; k chunk (4 kh + (l >> 4)) ^ (i & 6): k half 1 = bit 6 flipped
    const int fro = ((lane & 15) >> 3) * 1024 + (lane & 7) * 128 + (((lane >> 4) ^ (lane & 6)) << 4);
    const char* const rd0 = smem + fro;
    const char* const rd1 = smem + (fro ^ 64);

    f32x4 acc[RB][NCB];
#pragma unroll
    for (int a = 0; a < RB; ++a)
#pragma unroll
        for (int b = 0; b < NCB; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    bf16x8 a0[NA], a1[NA], a2[NA];                    // A register sets: [rb * 2 + kh]
    bf16x8 fx[CBP][2];                                // W fragments of the current phase (rolling, see D8_READ1)

#define D8_FENCE() __builtin_amdgcn_sched_barrier(0);
    // W fragment F[t][kh] of a phase = column block PH * CBP + t, k half kh.  ONE fragment set, rolling: step s = kh * CBP + t of a phase
    // issues the two MFMAs (row blocks 0, 1) of F[t][kh] and then re-requests the SAME registers for the next phase - the read has a whole
    // phase (4 CBP MFMAs) to land, reads and MFMAs alternate 1 : 2 instead of arriving in bursts, and no second fragment set is needed.
#define D8_READ1(T, KH, BOFF, PH) fx[T][KH] = *(const bf16x8*)(((KH) ? rd1 : rd0) + (BOFF) + ((PH) * CBP + (T)) * 2048);
#define D8_MFMA1(T, KH, AS, PH)                                                                                      \
    _Pragma("unroll") for (int rb = 0; rb < RB; ++rb)                                                                \
        acc[rb][(PH) * CBP + (T)] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fx[T][KH], AS[rb * 2 + (KH)], acc[rb][(PH) * CBP + (T)], 0, 0, 0);
    // One vector-memory instruction of this K-tile's group: slots 0 .. ND - 1 = the W pieces of K-tile u + 3 (into buffer DBUF), slots ND ..
    // ND + 3 = the A loads of K-tile u + 2 (into ANEW).  The slots are SPREAD over the phases, each between the two k halves of a phase's MFMAs:
    // issued together behind the barrier (the first build) the eight waves' 64 instructions queue at the texture path for ~1000 cycles during
    // which no wave reaches an MFMA (profiles/r5_gemm_d8.txt: every stream removed alone bought 9-18 %).
#define D8_SLOT(S, ANEW, DBUF)                                                                                       \
    if ((S) < ND) {                                                                                                  \
        const unsigned long long sb_ = wb[(S) < ND ? (S) : 0] + (unsigned long long)kW * 128;                        \
        const unsigned ld_ = lds0 + (DBUF) * BUFSZ + (wave * ND + (S)) * 1024;                                       \
        D8_DMA1(voffW, sb_, ld_)                                                                                     \
        if ((S) == ND - 1) D8_WRAP_W()                                                                               \
    } else if ((S) < ND + NA) {                                                                                      \
        const unsigned long long sa_ = ab + (unsigned long long)kA * 2048;                                           \
        if ((S) == ND) D8_LOADA(ANEW[0], voffA[0], sa_, 0)                                                           \
        if ((S) == ND + 1) D8_LOADA(ANEW[1], voffA[0], sa_, 1024)                                                    \
        if constexpr (RB == 2) {                                                                                     \
            if ((S) == ND + 2) D8_LOADA(ANEW[NA - 2], voffA[1], sa_, 0)                                              \
            if ((S) == ND + 3) D8_LOADA(ANEW[NA - 1], voffA[1], sa_, 1024)                                           \
        }                                                                                                            \
        if ((S) == ND + NA - 1) D8_WRAP_A()                                                                          \
    }
    // the ND + NA slots of a K-tile are spread evenly over its 2 NCB steps (one step = one W fragment = RB MFMAs): slot i sits behind
    // step ((2 i + 1) * 2 NCB) / (2 (ND + NA))
#define D8_STEP_SLOT(PH, S, ANEW, DBUF)                                                                              \
    _Pragma("unroll") for (int i_ = 0; i_ < ND + NA; ++i_)                                                           \
        if ((PH) * 2 * CBP + (S) == ((2 * i_ + 1) * 2 * NCB) / (2 * (ND + NA))) { D8_SLOT(i_, ANEW, DBUF) }
    // phase PH of a K-tile: RBUF / RPH = buffer offset and phase the re-requested fragments belong to
#define D8_PHASE(RBUF, RPH, ACUR, ANEW, PH, DBUF)                                                                    \
    _Pragma("unroll") for (int s_ = 0; s_ < 2 * CBP; ++s_) {                                                         \
        D8_MFMA1(s_ % CBP, s_ / CBP, ACUR, PH) D8_FENCE()                                                            \
        D8_READ1(s_ % CBP, s_ / CBP, RBUF, RPH) D8_FENCE()                                                           \
        D8_STEP_SLOT(PH, s_, ANEW, DBUF) D8_FENCE()                                                                  \
    }
#define D8_WAIT(ACUR)                                                                                                \
    if constexpr (RB == 2) asm volatile("s_waitcnt vmcnt(%4)" : "+v"(ACUR[0]), "+v"(ACUR[1]), "+v"(ACUR[2]), "+v"(ACUR[3]) : "n"(ND + NA) : "memory"); \
    else asm volatile("s_waitcnt vmcnt(%2)" : "+v"(ACUR[0]), "+v"(ACUR[1]) : "n"(ND + NA) : "memory");
    // One K-tile u.  ACUR: the A set it computes with; ANEW: the set K-tile u - 1 used, refilled for K-tile u + 2.  bufc = u & 3.
    //   wait: this wave's group of two K-tiles ago = { W pieces of K-tile u + 1, A of K-tile u } (the group of K-tile u - 1 stays in flight)
    //   barrier: every wave's pieces of K-tile u + 1 have landed, every wave is done with the buffer of K-tile u - 1
    //   NPH phases; the last one re-requests K-tile u + 1's first fragments (complete since the barrier above);
    //   this K-tile's group (W pieces of K-tile u + 3 into the buffer of K-tile u - 1, A of K-tile u + 2) is issued slot by slot
#define D8_KTILE(ACUR, ANEW)                                                                                         \
    {                                                                                                                \
        D8_WAIT(ACUR)                                                                                                \
        D8_FENCE() __builtin_amdgcn_s_barrier(); D8_FENCE()                                                          \
        const int cur_ = bufc * BUFSZ, nxt_ = ((bufc + 1) & 3) * BUFSZ, dbuf_ = (bufc + 3) & 3;                      \
        _Pragma("unroll") for (int pp_ = 0; pp_ < NPH; ++pp_) {                                                      \
            D8_PHASE((pp_ + 1 < NPH ? cur_ : nxt_), (pp_ + 1) % NPH, ACUR, ANEW, pp_, dbuf_)                         \
        }                                                                                                            \
        bufc = (bufc + 1) & 3;                                                                                       \
    }

    // prologue: W of K-tiles 0, 1, 2 and A of K-tiles 0, 1 in the order the steady state would have issued them
    int bufc = 0;
    D8_ISSUE_W(0)
    D8_ISSUE_W(1) D8_ISSUE_A(a0)
    D8_ISSUE_W(2) D8_ISSUE_A(a1)
    asm volatile("s_waitcnt vmcnt(%0)" :: "n"(2 * (ND + NA)) : "memory");
    D8_FENCE() __builtin_amdgcn_s_barrier(); D8_FENCE()
    _Pragma("unroll") for (int s_ = 0; s_ < 2 * CBP; ++s_) { D8_READ1(s_ % CBP, s_ / CBP, 0, 0) }
    D8_FENCE()

    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        // each cursor wraps exactly once per compute tile (nk >= 3 K-tiles, the cursors run 3 / 2 K-tiles ahead): the tile it enters then
        D8_SETUP_W(wbn, tW + (int)gridDim.x)
        D8_SETUP_A(abn, tA + (int)gridDim.x)
        for (int kt = 0; kt < nk; kt += 3) {
            D8_KTILE(a0, a2)
            D8_KTILE(a1, a0)
            D8_KTILE(a2, a1)
        }
        int tm, tn;
        tile_of_index(p, tile, ntiles, tm, tn);
        if ((EPI == 0 || EPI == 1) && p.c_packed) d8_epilogue_packed<BN, EPI, RB>(p, acc, tm * BM + wrb * 16, tn * BN, lane);
        else d8_epilogue<BN, EPI, RB>(p, acc, tm * BM + wrb * 16, tn * BN, lane, smem + SCR + wave * 4096);
        // BN = 256, row-operand epilogues: 128 accumulator registers + the A sets in flight + the next tile's first W fragments leave the
        // epilogue too few registers - it spilled, and every spill reload is a load behind a store (a full drain).  The fragments are read
        // AGAIN here instead of being kept across the epilogue (the buffer is complete since the last K-tile's barrier and is not refilled
        // before the next tile's second K-tile): the same values, 16 registers free in the epilogue.
        if constexpr (BN == 256 && (EPI == 2 || EPI == 3)) {
            D8_FENCE()
            _Pragma("unroll") for (int s_ = 0; s_ < 2 * CBP; ++s_) { D8_READ1(s_ % CBP, s_ / CBP, bufc * BUFSZ, 0) }
            D8_FENCE()
        }
#pragma unroll
        for (int a = 0; a < RB; ++a)
#pragma unroll
            for (int b = 0; b < NCB; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    // keep the last prefetched registers formally alive up to the drain (their loads are in flight until here)
    asm volatile("" :: "v"(a0[0]), "v"(a1[0]), "v"(a2[0]), "v"(fx[0][0]));
}

template <int BN, int EPI>
__global__ __launch_bounds__(512) void gemm_d8_kernel(const GemmArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    d8_body<BN, EPI, 2, 256>(p, smem);
}
// 192-row tiles: the two waves of a SIMD are the two roles (waves w and w + 4 share a SIMD: a workgroup's waves go to the SIMDs cyclically)
template <int BN, int EPI>
__global__ __launch_bounds__(512) void gemm_d8r192_kernel(const GemmArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if (__builtin_amdgcn_readfirstlane(threadIdx.x >> 6) < 4) d8_body<BN, EPI, 2, 192>(p, smem);
    else d8_body<BN, EPI, 1, 192>(p, smem);
}

template <int BN, int EPI, int BM>
int launch_d8_one(const GemmArgs& a, hipStream_t st) {
    constexpr int smem = 4 * BN * 128 + 8 * 4096;     // four W buffers + the epilogue scratch (160 KiB at BN = 256)
    void (*kern)(const GemmArgs);
    if constexpr (BM == 256) kern = gemm_d8_kernel<BN, EPI>;
    else kern = gemm_d8r192_kernel<BN, EPI>;
    static bool attr_done = false;
    if (!attr_done) {
        (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, smem);
        attr_done = true;
    }
    int grid = min(a.tiles_m * a.tiles_n, orv_num_cus());
    if (a.grid_cap > 0) grid = min(grid, a.grid_cap);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(512), smem, st, a);
    return orv_check_launch("orv_gemm_bf16");
}

}  // namespace

namespace orv_gemm {
int launch_d8(const GemmArgs& a, int bn, int epi, hipStream_t st, int bm) {
    if (!a.a_packed || (long)a.N * a.ldw * 2 >= (1L << 32) || a.K % 192 != 0 || a.lda != a.K) {
        orv_set_error("orv_gemm_bf16: the d8 kernel needs a packed A (a_packed, lda == K), K %% 192 == 0 and W below 4 GiB (lda=%ld N=%d ldw=%ld K=%d)",
                      a.lda, a.N, a.ldw, a.K);
        return ORV_EINVAL;
    }
    if (a.c_packed && (epi > 1 || a.ldc != a.N || a.c_rows > 0 || a.Y)) {
        orv_set_error("orv_gemm_bf16: packed C needs epilogue 0 / 1, ldc == N, no row map, no Y");
        return ORV_EINVAL;
    }
    if (epi == 2 || epi == 3) {
        // the row-operand epilogues keep output row numbers (row map included) in 32 bits at BN = 256, and the gated one divides them per lane
        // in 32 bits where a wave's rows touch more than two gate rows
        const long last = a.c_rows > 0 ? (long)((a.M - 1) / a.c_rows) * a.c_bstride + a.c_off + a.c_rows - 1 : (long)a.M - 1;
        if (last >= (1L << 31) || (epi == 2 && a.gate && a.seq <= 0)) {
            orv_set_error("orv_gemm_bf16: the row-operand epilogues need output rows below 2^31 and seq > 0 (last row %ld, seq=%d)", last, a.seq);
            return ORV_EINVAL;
        }
    }
    if (bm == 192) {
        // 192-row tiles (gemm_d8r192_kernel): the packed A (and packed C) buffers hold orv_packed_rows(M) = ceil(M / 256) * 256 row slots and
        // neither the A loads nor the packed store are masked - the 192-row tiling must stay inside them (the chooser checks the same)
        if ((long)a.tiles_m * 192 > ((long)a.M + 255) / 256 * 256) {
            orv_set_error("orv_gemm_bf16: 192-row d8 tiles would read past the packed row slots (M=%d)", a.M);
            return ORV_EINVAL;
        }
        if (bn == 128) {
            switch (epi) {
                case 0: return launch_d8_one<128, 0, 192>(a, st);
                case 1: return launch_d8_one<128, 1, 192>(a, st);
                case 2: return launch_d8_one<128, 2, 192>(a, st);
                case 4: return launch_d8_one<128, 4, 192>(a, st);
            }
        } else if (bn == 192) {
            switch (epi) {
                case 0: return launch_d8_one<192, 0, 192>(a, st);
                case 1: return launch_d8_one<192, 1, 192>(a, st);
                case 2: return launch_d8_one<192, 2, 192>(a, st);
                case 4: return launch_d8_one<192, 4, 192>(a, st);
            }
        }
        orv_set_error("orv_gemm_bf16: no 192-row d8 kernel for BN=%d epilogue %d", bn, epi);
        return ORV_EINVAL;
    }
    if (bn == 256) {
        switch (epi) {
            case 0: return launch_d8_one<256, 0, 256>(a, st);
            case 1: return launch_d8_one<256, 1, 256>(a, st);
            case 2: return launch_d8_one<256, 2, 256>(a, st);
            case 3: return launch_d8_one<256, 3, 256>(a, st);
            case 4: return launch_d8_one<256, 4, 256>(a, st);
        }
    } else if (bn == 128) {
        switch (epi) {
            case 0: return launch_d8_one<128, 0, 256>(a, st);
            case 1: return launch_d8_one<128, 1, 256>(a, st);
            case 2: return launch_d8_one<128, 2, 256>(a, st);
            case 4: return launch_d8_one<128, 4, 256>(a, st);
        }
    } else if (bn == 192) {
        switch (epi) {
            case 0: return launch_d8_one<192, 0, 256>(a, st);
            case 1: return launch_d8_one<192, 1, 256>(a, st);
            case 2: return launch_d8_one<192, 2, 256>(a, st);
            case 3: return launch_d8_one<192, 3, 256>(a, st);
            case 4: return launch_d8_one<192, 4, 256>(a, st);
        }
    }
    orv_set_error("orv_gemm_bf16: no d8 kernel for BN=%d epilogue %d", bn, epi);
    return ORV_EINVAL;
}
}  // namespace orv_gemm

// ---- P16 pack / unpack (include/orv_mi355.h).  One thread per 16-byte piece, destination-ordered (coalesced writes). ----
namespace {
__global__ __launch_bounds__(256) void pack_rows16_kernel(const bf16_t* src, long ld, uint4* dst, int M, int K, long pieces) {
    const long d = (long)blockIdx.x * 256 + threadIdx.x;
    if (d >= pieces) return;
    const long blk = d >> 6;
    const int l = (int)(d & 63), kb = K / 32;
    const long row = (blk / kb) * 16 + (l & 15);
    const int k = (int)(blk % kb) * 32 + (l >> 4) * 8;
    dst[d] = row < M ? *(const uint4*)(src + row * ld + k) : make_uint4(0, 0, 0, 0);
}
__global__ __launch_bounds__(256) void unpack_rows16_kernel(const uint4* src, bf16_t* dst, long ld, int M, int K, long pieces) {
    const long d = (long)blockIdx.x * 256 + threadIdx.x;       // destination-ordered: piece d = (row, 8-column chunk)
    if (d >= pieces) return;
    const int kc = K / 8;
    const long row = d / kc;
    const int c = (int)(d % kc);
    const long blk = (row >> 4) * (K / 32) + (c >> 2);
    *(uint4*)(dst + row * ld + c * 8) = src[blk * 64 + (c & 3) * 16 + (row & 15)];
}
}  // namespace
extern "C" long orv_packed_rows(long rows) { return (rows + 255) / 256 * 256; }
extern "C" int orv_pack_rows16(const void* src, long ld_src, void* dst, int M, int K, void* stream) {
    ORV_REQUIRE(src && dst && M > 0 && K > 0 && K % 32 == 0 && ld_src % 8 == 0, "orv_pack_rows16: bad arguments (M=%d K=%d ld=%ld)", M, K, ld_src);
    const long pieces = orv_packed_rows(M) * (K / 8);
    hipLaunchKernelGGL(pack_rows16_kernel, dim3((unsigned)((pieces + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)src, ld_src,
                       (uint4*)dst, M, K, pieces);
    return orv_check_launch("orv_pack_rows16");
}
extern "C" int orv_unpack_rows16(const void* src, void* dst, long ld_dst, int M, int K, void* stream) {
    ORV_REQUIRE(src && dst && M > 0 && K > 0 && K % 32 == 0 && ld_dst % 8 == 0, "orv_unpack_rows16: bad arguments (M=%d K=%d ld=%ld)", M, K, ld_dst);
    const long pieces = (long)M * (K / 8);
    hipLaunchKernelGGL(unpack_rows16_kernel, dim3((unsigned)((pieces + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const uint4*)src,
                       (bf16_t*)dst, ld_dst, M, K, pieces);
    return orv_check_launch("orv_unpack_rows16");
}
