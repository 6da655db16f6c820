// Epilogue of the LDS-staged GEMM kernels (gemm.hip: simple / ring / phased / convolution kernels; gemm_mxfp8.hip: the MXFP8
// kernel), shared so that every kernel with the 32x32 C^T accumulator layout below stores through one copy of it.
#pragma once
#include "gemm_common.hpp"

namespace {

using namespace orv_gemm;

// Epilogue shared by both kernels.  acc[i][j][4q+e] = C[m][n] with m = mbase + j*32 + (lane&31),
// n = nbase + i*32 + 8q + 4*(lane>>5) + e  (C^T accumulator layout: 4 consecutive columns per register quad).
// Memory side: lanes l and l+32 own the two 8-byte halves of one 16-byte column group of the SAME row, so two column
// groups (register quads 2u, 2u+1) are exchanged with v_permlane32_swap and every lane moves ONE aligned 16-byte piece
// (lower half-wave: group 2u, upper: group 2u+1): half the store/load instructions of the 8-byte form and 32
// contiguous bytes per row and instruction (measured: the 8-byte stores cost 15 % of the FFN1 GEMM).
__device__ __forceinline__ void swap_halves(uint32_t& a, uint32_t& b) {
    // a of the upper half-wave <-> b of the lower half-wave
    const auto r = __builtin_amdgcn_permlane32_swap(a, b, false, false);
    a = r[0]; b = r[1];
}

__device__ __forceinline__ float sum_with_partner_half(float v) {   // v(lane) + v(lane ^ 32)
    const unsigned u = __float_as_uint(v);
    const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
// two register quads (this lane's 4 columns of column groups 2u and 2u+1) -> one aligned 16-byte piece per lane
__device__ __forceinline__ void store_quads16(bf16_t* row, int n16, const float (&a)[4], const float (&b)[4]) {
    uint32_t a0 = pack2bf(a[0], a[1]), a1 = pack2bf(a[2], a[3]), b0 = pack2bf(b[0], b[1]), b1 = pack2bf(b[2], b[3]);
    swap_halves(a0, b0);
    swap_halves(a1, b1);
    *(uint4*)(row + n16) = make_uint4(a0, a1, b0, b1);
}

// Epilogue 4: the QKV projection with the per-head LayerNorm(64) of q and k (diffusers Attention.norm_q / norm_k as called
// at cogvideox_control.py:243-247) and the softmax pre-multiplier of q applied in registers; the v third is stored as is.
// A wave's BN/2 columns are whole heads of ONE of q | k | v (host-checked), a head is two adjacent 32-column blocks, and
// a row's 64 values sit in this lane (32) and lane ^ 32 (32): the statistics are lane-local sums plus one half-wave swap.
// Optional Y keeps acc + bias (the raw projection) for the LayerNorm adjoint.
template <int NB, int MB>
__device__ __forceinline__ void gemm_epilogue_qknorm(const GemmArgs& p, f32x16 (&acc)[NB][MB], int mbase, int nbase, int lane) {
    static_assert(NB % 2 == 0, "a wave must cover whole 64-wide heads");
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const int l31 = lane & 31, hi = lane >> 5;
    const int region = __builtin_amdgcn_readfirstlane(nbase / (p.qn_heads * 64));   // 0 = q, 1 = k, 2 = v
    const bf16_t* gam = region == 0 ? p.qn_gq : p.qn_gk;
    const bf16_t* bet = region == 0 ? p.qn_bq : p.qn_bk;
    const float post = region == 0 ? p.qn_premul : 1.f;
    // One head (two 32-column blocks of one row block) at a time, fenced with sched_barrier: the 192 accumulator registers
    // leave no room for the scheduler to overlap heads (it did, and spilled ~700 registers).
#pragma unroll
    for (int j = 0; j < MB; ++j) {
        const int m = mbase + j * 32 + l31;
        const bool valid = m < p.M;               // lane and lane ^ 32 hold the same row
        bf16_t* crow = p.C + (long)min(m, p.M - 1) * p.ldc;
        bf16_t* yrow = p.Y ? p.Y + (long)min(m, p.M - 1) * p.ldy : nullptr;
#pragma unroll
        for (int hh = 0; hh < NB / 2; ++hh) {
            __builtin_amdgcn_sched_barrier(0);
            float v[2][16];
#pragma unroll
            for (int ii = 0; ii < 2; ++ii)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    float bb[4] = {0.f, 0.f, 0.f, 0.f};
                    if (p.bias) {
                        const int nq = __builtin_amdgcn_readfirstlane(nbase + (2 * hh + ii) * 32 + q * 8);
                        const u32x4 b8 = *(const __attribute__((address_space(4))) u32x4*)(uintptr_t)(p.bias + nq);
                        const uint32_t bx = hi ? b8[2] : b8[0], by = hi ? b8[3] : b8[1];
                        bb[0] = bf2f(bx & 0xffff); bb[1] = bf2f(bx >> 16); bb[2] = bf2f(by & 0xffff); bb[3] = bf2f(by >> 16);
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[ii][q * 4 + e] = acc[2 * hh + ii][j][q * 4 + e] + bb[e];
                }
            if (yrow) {
#pragma unroll
                for (int ii = 0; ii < 2; ++ii)
#pragma unroll
                    for (int u = 0; u < 2; ++u) {
                        float a[4], b[4];
#pragma unroll
                        for (int e = 0; e < 4; ++e) { a[e] = v[ii][(2 * u) * 4 + e]; b[e] = v[ii][(2 * u + 1) * 4 + e]; }
                        if (valid) store_quads16(yrow, nbase + (2 * hh + ii) * 32 + (2 * u + hi) * 8, a, b);
                    }
            }
            if (region < 2) {
                float s = 0.f;
#pragma unroll
                for (int ii = 0; ii < 2; ++ii)
#pragma unroll
                    for (int r = 0; r < 16; ++r) s += v[ii][r];
                const float mean = sum_with_partner_half(s) * (1.f / 64.f);
                float sq = 0.f;
#pragma unroll
                for (int ii = 0; ii < 2; ++ii)
#pragma unroll
                    for (int r = 0; r < 16; ++r) { v[ii][r] -= mean; sq += v[ii][r] * v[ii][r]; }
                const float rstd = rsqrtf(sum_with_partner_half(sq) * (1.f / 64.f) + p.qn_eps);
#pragma unroll
                for (int ii = 0; ii < 2; ++ii)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        float g[4] = {1.f, 1.f, 1.f, 1.f}, bb[4] = {0.f, 0.f, 0.f, 0.f};
                        if (gam) {
                            const u32x4 g8 = *(const __attribute__((address_space(4))) u32x4*)(uintptr_t)(gam + ii * 32 + q * 8);
                            const uint32_t gx = hi ? g8[2] : g8[0], gy = hi ? g8[3] : g8[1];
                            g[0] = bf2f(gx & 0xffff); g[1] = bf2f(gx >> 16); g[2] = bf2f(gy & 0xffff); g[3] = bf2f(gy >> 16);
                        }
                        if (bet) {
                            const u32x4 b8 = *(const __attribute__((address_space(4))) u32x4*)(uintptr_t)(bet + ii * 32 + q * 8);
                            const uint32_t bx = hi ? b8[2] : b8[0], by = hi ? b8[3] : b8[1];
                            bb[0] = bf2f(bx & 0xffff); bb[1] = bf2f(bx >> 16); bb[2] = bf2f(by & 0xffff); bb[3] = bf2f(by >> 16);
                        }
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[ii][q * 4 + e] = (v[ii][q * 4 + e] * rstd * g[e] + bb[e]) * post;
                    }
            }
#pragma unroll
            for (int ii = 0; ii < 2; ++ii)
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    float a[4], b[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) { a[e] = v[ii][(2 * u) * 4 + e]; b[e] = v[ii][(2 * u + 1) * 4 + e]; }
                    if (valid) store_quads16(crow, nbase + (2 * hh + ii) * 32 + (2 * u + hi) * 8, a, b);
                }
        }
    }
    __builtin_amdgcn_sched_barrier(0);
}

template <int NB, int MB, int EPI>
__device__ __forceinline__ void gemm_epilogue(const GemmArgs& p, f32x16 (&acc)[NB][MB], int mbase, int nbase, int lane) {
    if constexpr (EPI == 4) {
        gemm_epilogue_qknorm<NB, MB>(p, acc, mbase, nbase, lane);
        return;
    }
    const int l31 = lane & 31, hi = lane >> 5;
#pragma unroll
    for (int j = 0; j < MB; ++j) {
        const int m = mbase + j * 32 + l31;
        if (m >= p.M) continue;
        long orow = m;
        if (p.c_rows > 0) orow = (long)(m / p.c_rows) * p.c_bstride + p.c_off + m % p.c_rows;
        bf16_t* crow = p.C + orow * p.ldc;
        bf16_t* yrow = p.Y ? p.Y + orow * p.ldy : nullptr;
        const bf16_t* rrow = nullptr;
        const float* grow = nullptr;
        if (EPI == 2 || EPI == 3) {
            const long rr = p.r_mod > 0 ? m % p.r_mod : orow;
            rrow = p.R + rr * p.ldr;
            if (p.gate) {
                const int bidx = (int)(orow / p.seq), s = (int)(orow % p.seq);
                grow = p.gate + bidx * p.gate_b + orv_group_of(s, p.n_text, p.per_group) * p.gate_g;
            }
        }
        // Every vector load issued here queues BEHIND the DMA pieces already in flight for the next tile (vmcnt retires in
        // order), i.e. costs a full loaded-memory-pipeline latency: so the bias comes through the scalar cache (uniform
        // address, s_load), and the per-row operands (residual, gate) of a row block are all requested up front.
        constexpr int IB = NB <= 4 ? NB : 2;   // blocks whose row operands are requested together (register budget)
        bool g_uniform = false;     // all rows of this 32-row block share one gate row -> gate through the scalar cache too
        const float* g_srow = nullptr;
        if (EPI == 2 && p.gate) {
            const int mf = __builtin_amdgcn_readfirstlane(mbase + j * 32), ml = min(mf + 31, p.M - 1);
            long of = mf, ol = ml;
            if (p.c_rows > 0) {
                of = (long)(mf / p.c_rows) * p.c_bstride + p.c_off + mf % p.c_rows;
                ol = (long)(ml / p.c_rows) * p.c_bstride + p.c_off + ml % p.c_rows;
            }
            const int bf_ = (int)(of / p.seq), bl_ = (int)(ol / p.seq);
            const int gf_ = orv_group_of((int)(of % p.seq), p.n_text, p.per_group);
            const int gl_ = orv_group_of((int)(ol % p.seq), p.n_text, p.per_group);
            g_uniform = (bf_ == bl_) && (gf_ == gl_);
            g_srow = p.gate + bf_ * p.gate_b + gf_ * p.gate_g;
        }
#pragma unroll
        for (int i0 = 0; i0 < NB; i0 += IB) {
        uint32_t rq[IB][2][2][2];   // [block][u][quad t][dword]: residual / pre-activation operand, this lane's 4 columns
        if (EPI == 2 || EPI == 3) {
#pragma unroll
            for (int ii = 0; ii < IB; ++ii)
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const uint4 rr = *(const uint4*)(rrow + nbase + (i0 + ii) * 32 + (2 * u + hi) * 8);
                    rq[ii][u][0][0] = rr.x; rq[ii][u][0][1] = rr.y; rq[ii][u][1][0] = rr.z; rq[ii][u][1][1] = rr.w;
                }
#pragma unroll
            for (int ii = 0; ii < IB; ++ii)
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    // loaded: lower = group 2u cols 0-7, upper = group 2u+1 cols 0-7  ->  (quad 2u | quad 2u+1) own 4 columns
                    swap_halves(rq[ii][u][0][0], rq[ii][u][1][0]);
                    swap_halves(rq[ii][u][0][1], rq[ii][u][1][1]);
                }
        }
#pragma unroll
        for (int ii = 0; ii < IB; ++ii) {
            const int i = i0 + ii;
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                // this lane's 16-byte piece: column group 2u + hi of the 32-column block
                const int n16 = nbase + i * 32 + (2 * u + hi) * 8;
                uint32_t oc[2][2], oy[2][2];
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const int q = 2 * u + t;
                    float v[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = acc[i][j][q * 4 + e];
                    if (p.bias) {
                        const int nq = __builtin_amdgcn_readfirstlane(nbase + i * 32 + q * 8);   // wave-uniform + constant address space: s_load
                        typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
                        const u32x4 b8 = *(const __attribute__((address_space(4))) u32x4*)(uintptr_t)(p.bias + nq);
                        const uint32_t bx = hi ? b8[2] : b8[0], by = hi ? b8[3] : b8[1];
                        v[0] += bf2f(bx & 0xffff); v[1] += bf2f(bx >> 16);
                        v[2] += bf2f(by & 0xffff); v[3] += bf2f(by >> 16);
                    }
                    if (yrow) {   // training: keep acc + bias (GELU pre-activation / un-gated branch output)
                        oy[t][0] = pack2bf(v[0], v[1]); oy[t][1] = pack2bf(v[2], v[3]);
                    }
                    if (EPI == 1) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = gelu_tanh(v[e]);
                    }
                    if (EPI == 2) {
                        float g[4] = {1.f, 1.f, 1.f, 1.f};
                        if (grow) {
                            if (g_uniform) {
                                typedef float f32x4s __attribute__((ext_vector_type(4)));
                                const int nq = __builtin_amdgcn_readfirstlane(nbase + i * 32 + q * 8);
                                const f32x4s ga = *(const __attribute__((address_space(4))) f32x4s*)(uintptr_t)(g_srow + nq);
                                const f32x4s gb = *(const __attribute__((address_space(4))) f32x4s*)(uintptr_t)(g_srow + nq + 4);
#pragma unroll
                                for (int e = 0; e < 4; ++e) g[e] = hi ? gb[e] : ga[e];
                            } else {   // block straddles a frame / text boundary (about 1 in 19): per-row gate rows
                                const float4 gg = *(const float4*)(grow + nbase + i * 32 + q * 8 + hi * 4);
                                g[0] = gg.x; g[1] = gg.y; g[2] = gg.z; g[3] = gg.w;
                            }
                        }
                        v[0] = bf2f(rq[ii][u][t][0] & 0xffff) + g[0] * v[0]; v[1] = bf2f(rq[ii][u][t][0] >> 16) + g[1] * v[1];
                        v[2] = bf2f(rq[ii][u][t][1] & 0xffff) + g[2] * v[2]; v[3] = bf2f(rq[ii][u][t][1] >> 16) + g[3] * v[3];
                    }
                    if (EPI == 3) {   // backward through GELU(tanh): C = acc * gelu'(U), U = saved pre-activation
                        v[0] *= gelu_tanh_grad(bf2f(rq[ii][u][t][0] & 0xffff)); v[1] *= gelu_tanh_grad(bf2f(rq[ii][u][t][0] >> 16));
                        v[2] *= gelu_tanh_grad(bf2f(rq[ii][u][t][1] & 0xffff)); v[3] *= gelu_tanh_grad(bf2f(rq[ii][u][t][1] >> 16));
                    }
                    oc[t][0] = pack2bf(v[0], v[1]); oc[t][1] = pack2bf(v[2], v[3]);
                }
                if (yrow) {
                    swap_halves(oy[0][0], oy[1][0]);
                    swap_halves(oy[0][1], oy[1][1]);
                    *(uint4*)(yrow + n16) = make_uint4(oy[0][0], oy[0][1], oy[1][0], oy[1][1]);
                }
                swap_halves(oc[0][0], oc[1][0]);   // lower: (A cols 0-3 | A cols 4-7) ; upper: (B cols 0-3 | B cols 4-7)
                swap_halves(oc[0][1], oc[1][1]);
                *(uint4*)(crow + n16) = make_uint4(oc[0][0], oc[0][1], oc[1][0], oc[1][1]);
            }
        }
        }
    }
}

}  // namespace
