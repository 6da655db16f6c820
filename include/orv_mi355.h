/*
 * liborv_mi355.so - C ABI of the MI355X (gfx950) kernels behind the ORV denoising hot path.
 *
 * The reference (OrangeSodahub/ORV) has no FFI seam on this path: it is nn.Module Python calling torch
 * (SURVEY.md §8b).  This header is the seam the replacement introduces *beneath* the reference's Python
 * surface; every entry point cites the reference code whose arithmetic it replaces
 * (paths relative to /root/reference).  The Python binding a maintainer adds is in INTEGRATION.md.
 *
 * Conventions
 *  - All pointers are DEVICE pointers borrowed from the caller (torch tensors); the library never
 *    allocates or frees caller memory.  bf16 tensors are passed as `const void*` to 2-byte elements.
 *  - Every call is stream-ordered and asynchronous on `stream` (a hipStream_t passed as void*;
 *    callers pass torch.cuda.current_stream().cuda_stream).  No internal synchronisation.
 *  - Return value: 0 = ok, <0 = error (ORV_E*); never throws.  `orv_last_error()` returns a
 *    thread-local message for the last failing call on this thread.
 *  - "Token group" indexing (per-frame modulation, cogvideox_control.py:99-105,133-140):
 *      row s of a [B, S, D] joint sequence (text first) belongs to group
 *      g(s) = 0                      if s <  n_text
 *             1 + (s - n_text) / P   otherwise           (P = tokens per latent frame)
 *    and modulation tables are fp32 [B, G, D] slices with explicit strides.
 */
#ifndef ORV_MI355_H
#define ORV_MI355_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ORV_OK 0
#define ORV_EINVAL (-1)   /* bad argument / unsupported shape */
#define ORV_EDEVICE (-2)  /* not a gfx950 device / HIP failure */
#define ORV_ELAUNCH (-3)  /* kernel launch failed */

/* -- library ---------------------------------------------------------------------------------- */
int orv_version(void);                 /* ABI version, currently 1 */
const char* orv_last_error(void);      /* thread-local message of the last failing call */
int orv_device_check(int device);      /* 0 iff `device` is gfx950 (MI355X) */

/* Token-group descriptor shared by the modulation-aware kernels. */
typedef struct {
    int seq;        /* S: rows per batch element */
    int n_text;     /* rows [0, n_text) are text rows (group 0) */
    int per_group;  /* P: video rows per group; 0 => all video rows are group 1 */
} orv_groups_t;

/* Row remap r -> (r / rows) * bstride + off + r % rows (rows == 0: identity).  Lets a kernel read or write the video
 * (or text) rows of the joint [B, S, D] sequence in place instead of materialising torch.cat / slices
 * (cogvideox_control.py:222,267-269,437-443,792-794). */
typedef struct {
    int rows, bstride, off;
} orv_rowmap_t;

/* -- embeddings ------------------------------------------------------------------------------- */
/* diffusers Timesteps(dim, flip_sin_to_cos, shift) as called at orv/models/cogvideox_control.py:763,772:
 * out[b] = [cos(t*f) | sin(t*f)] (flip) with f_k = exp(-ln(1e4) k / (dim/2 - shift)); fp32 math, bf16 out. */
int orv_timestep_embedding(const float* t, void* out_bf16, int batch, int dim, int flip_sin_to_cos,
                           float freq_shift, void* stream);

/* Small-M linear (M <= 64): out[m, :] = act_out( W . act_in(x[m] + xb[m / xb_rep]) + bias ).
 * Replaces the tiny MLPs/linears of time_embedding (:769), ActionEmbed (components.py:37-45,65),
 * ActionRecon (components.py:86-90) and the AdaLN modulation linears (:121-130, :172).
 * x [M,K] bf16; xb optional [ceil(M/xb_rep), K] bf16 broadcast-added before act_in; W [N,K] bf16; bias [N] bf16|NULL.
 * act: 0 none, 1 SiLU, 2 GELU(tanh).  out_f32 != 0 -> fp32 output else bf16.  ldo = output row stride (elements); omap remaps output rows. */
int orv_skinny_linear(const void* x, const void* xb, int xb_rep, const void* W, const void* bias, void* out,
                      int M, int N, int K, int act_in, int act_out, int out_f32, int ldo, orv_rowmap_t omap,
                      void* stream);

/* Gather [B,T,C,H,W] latents into patch tokens (diffusers CogVideoXPatchEmbed.forward patchify, called at
 * cogvideox_control.py:788,833,842).  Two channel-concatenated sources (cogvideox_control.py:1409-1413 cat on dim 2)
 * are read in place: channels [0,c0) from src0, [c0,c0+c1) from src1 (src1 may be NULL with c1 = 0).
 * pt == 0: tokens [B, T*h*w, (C, p, p)]      (Conv2d weight.flatten(1) order)
 * pt  > 0: tokens [B, T/pt*h*w, (C, pt, p, p)]  (CogVideoX1.5 Linear order).  Index-exact (bit copies). */
int orv_patchify(const void* src0, int c0, const void* src1, int c1, void* tokens, int B, int T, int H, int W,
                 int p, int pt, void* stream);

/* Inverse scatter of cogvideox_control.py:926-936: x [B, N, p*p*(pt)*C] -> out [B,T,C,H,W].  Index-exact. */
int orv_unpatchify(const void* x, void* out, int B, int T, int C, int H, int W, int p, int pt, void* stream);

/* out[m, col_off + d] = a[amap(m), d] + b[m, d] (bf16, fp32 add, one rounding): builds the input of
 * initial_combine_linear, `hidden_states.repeat(1, 1, num_control_keys) + cat(controls, -1)` (cogvideox_control.py:849-855),
 * one control key per call, reading the video rows of the joint sequence in place. */
int orv_add_rows(const void* a, int lda, orv_rowmap_t amap, const void* b, int ldb, void* out, int ldo, int col_off, int M,
                 int D, void* stream);

/* Multiview cross-view attention (MVBlock.forward cogvideox_control.py:313-348) re-groups tokens
 * '(b v) (f s) d -> (b f) (v s) d' (einops rearrange :328,:346; text '(b v) n d -> (b f) (v n) d' :329-331):
 * orv_gather_rows:        dst[r, :] = src[idx[r], :]                      (idx = host-built permutation, int32 on device)
 * orv_scatter_gated_rows: x[idx[r], :] += gate[idx[r] / seq, :] * y[r, :]  for video target rows only - the rearrange back
 *                         fused with the gated residual `hidden + gate_msa * attn` (:347). */
int orv_gather_rows(const void* src, int ld_src, const int* idx, void* dst, int ld_dst, int R, int D, void* stream);
int orv_scatter_gated_rows(const void* y, int ldy, const int* idx, const float* gate, long gate_b, void* x, int ldx, int R,
                           int D, int seq, int n_text, void* stream);

/* -- normalisation ---------------------------------------------------------------------------- */
/* y = LN(x; gamma, beta, eps) * (1 + scale[b, g(s)]) + shift[b, g(s)]   (CogVideoXLayerNormZero.forward
 * cogvideox_control.py:117-145, AdaLayerNorm.forward :155-197, nn.LayerNorm norm_final :909-916).
 * x,y [B*S, D] bf16 (row strides ldx/ldy elements); gamma/beta bf16 [D] or NULL; scale/shift fp32 with
 * element strides (mod_b, mod_g) or NULL (plain LayerNorm).  Statistics in fp32.  Row r of the [batch*grp.seq] problem is
 * read from x row xmap(r) and written to y row r. */
int orv_layernorm_modulate(const void* x, int ldx, orv_rowmap_t xmap, void* y, int ldy, const void* gamma,
                           const void* beta, const float* scale, const float* shift, long mod_b, long mod_g,
                           orv_groups_t grp, int batch, int D, float eps, void* stream);
/* The same with y written in the packed P16 layout (orv_gemm_t: orv_packed_rows(batch * seq) x D bf16) - the A operand of the projections that
 * follow a CogVideoXLayerNormZero (cogvideox_control.py:232-234, 439) on the d8 GEMM.  Full case only (gamma, beta, scale, shift given, no row
 * map), D % 32 == 0, D <= 2048. */
int orv_layernorm_modulate_packed(const void* x, int ldx, void* y, const void* gamma, const void* beta, const float* scale,
                                  const float* shift, long mod_b, long mod_g, orv_groups_t grp, int batch, int D, float eps,
                                  void* stream);

/* All AdaLN modulation linears of one forward in a single launch (CogVideoXLayerNormZero "partially forward self.linear
 * twice" cogvideox_control.py:117-130, and AdaLayerNorm :172): for tab in [0, n_tab)
 *   out[tab][b][1+t][:] = W[tab][0:width]       . SiLU(temb[b] + action_emb[b,t]) + bias[tab][0:width]
 *   out[tab][b][0][:]   = W[tab][width:2*width] . SiLU(temb[b])                   + bias[tab][width:2*width]   (if text)
 * temb [B,E] bf16, action_emb [B,T,E] bf16 or NULL (then T must be 1 and the video rows use SiLU(temb)); W/bias are DEVICE
 * arrays of n_tab device pointers to bf16 [width*(1+text), E] / [width*(1+text)] (bias array or entries may be NULL);
 * out fp32 [n_tab, B, 1+T, width].  E in {64,128,256,512}, width % 32 == 0.  Streams every weight once (HBM-bound). */
int orv_modulation_tables(const void* temb, const void* action_emb, const void* const* W, const void* const* bias,
                          float* out, int n_tab, int B, int T, int E, int width, int text, void* stream);

/* In-place per-head LayerNorm(64, eps) on the q and k thirds of a packed qkv buffer [B*S, 3*H*64] bf16, optional
 * RoPE on rows >= n_text (pairs (2i,2i+1); cos/sin fp32 [S-n_text, 64]), and transpose of the v third into
 * vT [B, H, 64, s_pad] (zero-filled for s >= S; the key axis is stored with bits 2 and 3 of the key index exchanged,
 * the order orv_attention_fwd's PV MFMA consumes).  q is multiplied by `q_premul` before its single bf16 rounding: pass
 * softmax_scale * log2(e) and call orv_attention_fwd with scale = softmax_scale / q_premul to take its fused exp2 path
 * (1.0f = leave q as is).  Replaces cogvideox_control.py:239-254 (+ diffusers Attention.norm_q/norm_k,
 * apply_rotary_emb). */
int orv_qkv_prep(void* qkv, void* vT, const void* gq, const void* bq, const void* gk, const void* bk,
                 const float* rope_cos, const float* rope_sin, int B, int S, int H, int n_text, int s_pad,
                 float eps, float q_premul, void* stream);
/* Out-of-place form (training keeps the raw QKV GEMM output for the qk-LayerNorm adjoint): reads `src`, writes the
 * normalised q / k and the untouched v third to `qkv`.  src == qkv is the in-place call above. */
int orv_qkv_prep_from(const void* src, void* qkv, void* vT, const void* gq, const void* bq, const void* gk, const void* bk,
                      const float* rope_cos, const float* rope_sin, int B, int S, int H, int n_text, int s_pad, float eps,
                      float q_premul, void* stream);

/* -- GEMM ------------------------------------------------------------------------------------- */
/* C = epilogue(A[M,K] . W[N,K]^T + bias[N]); bf16 operands, fp32 MFMA accumulation, bf16 output.
 * Replaces nn.Linear / Conv2d(k=s=p) on the path: to_q/k/v + to_out (cogvideox_control.py:232-234,263),
 * FeedForward (:439-440), text_proj/proj (:788), proj_out (:920), initial_combine_linear (:853).
 * epilogue: 0 bias; 1 bias+GELU(tanh) (FeedForward net.0); 2 C = R[r_row] + gate[b,g(row)] * (acc + bias)
 * (gated residual :419-421,442-443; gate NULL => 1; R row r_row = r_mod ? m % r_mod : out_row, so a
 * [n,D] table broadcast over the batch - the sincos pos-embedding - uses r_mod = n).
 * epilogue 3 (backward): C = acc * GELU'(R[out_row]) - the dgrad of FeedForward net.2 fused with the GELU adjoint
 * (R = saved pre-activation).  Epilogue 2 with gate NULL and R == C accumulates gradients in place.
 * epilogue 4: the packed QKV projection with the qk LayerNorm fused (see the qn_* fields).
 * Output row remap: out_row = cmap(m) (scatter into the joint [B,S,D] sequence).  Constraints: K % 64 == 0, N % 64 == 0, 16-byte aligned rows. */
typedef struct {
    const void* A; int lda;
    const void* W; int ldw;
    const void* bias;
    void* C; int ldc;
    int M, N, K;
    int epilogue;
    const void* R; int ldr; int r_mod;
    const float* gate; long gate_b, gate_g; orv_groups_t grp;
    orv_rowmap_t cmap;
    void* Y; int ldy;   /* optional: also store acc + bias (before GELU / gate) at the same rows - saved for backward */
    /* epilogue 4 only - the packed QKV projection [M, 3*heads*64] with the per-head LayerNorm(64, eps) of the q and k
     * thirds (affine [64] bf16 or NULL) fused, q additionally multiplied by qn_premul, v stored as is; Y (if given)
     * receives the raw projection.  Equivalent to epilogue 0 followed by orv_qkv_prep without RoPE, minus the V^T copy
     * (use orv_head_transpose for that). */
    const void *qn_gamma_q, *qn_beta_q, *qn_gamma_k, *qn_beta_k; float qn_eps, qn_premul; int qn_heads;
    /* Packed operand layout "P16" (round 5, gemm_d8.hip).  A [rows, cols] bf16 matrix (cols % 32 == 0) stored as 1-KiB blocks of 16 rows x 32
     * columns, block (R, c) at byte ((R * cols / 32) + c) * 1024, element (r, k) of a block at ((k / 8) * 16 + r) * 16 + (k % 8) * 2 - the
     * order in which one wave instruction of v_mfma_f32_16x16x32_bf16 wants a 16 x 32 operand, so a GEMM reads its A operand straight into
     * registers with contiguous 1-KiB loads.  The buffer holds orv_packed_rows(rows) = rows rounded up to 256 row slots (padding rows are
     * never interpreted).  a_packed: A is in that layout (lda == K; needs K % 192 == 0); c_packed: C is written in it (ldc == N; epilogues
     * 0 / 1, no cmap / Y) - the FeedForward hidden state between cogvideox_control.py:439 and :440 never exists row-major.  Producers:
     * orv_pack_rows16, orv_layernorm_modulate (out_packed), orv_gemm_bf16 (c_packed), orv_attention_fwd* (out_packed). */
    int a_packed, c_packed;
} orv_gemm_t;
int orv_gemm_bf16(const orv_gemm_t* g, void* stream);
/* Row slots of a packed P16 buffer for `rows` rows (rounded up to the 256-row GEMM tile). */
long orv_packed_rows(long rows);
/* dst (P16 layout, orv_packed_rows(M) x K) = src [M, K] row-major (ld_src elements per row), bit copies; padding rows are zero-filled.
 * The reference has no such step (its operands stay row-major inside torch.nn.functional.linear, cogvideox_control.py:232-234,263,439-440):
 * this is the entry of tensors that no packed-writing kernel produced (tests, the first GEMM after a foreign op). */
int orv_pack_rows16(const void* src, long ld_src, void* dst, int M, int K, void* stream);
/* Inverse of orv_pack_rows16 (rows [0, M)). */
int orv_unpack_rows16(const void* src, void* dst, long ld_dst, int M, int K, void* stream);
/* Kernel symbol (as rocprofv3 prints it, e.g. "gemm_pp_kernel<192, 5, 1>") that orv_gemm_bf16 launches for this shape on this
 * device: the tile is chosen by a cost model over all candidates, so callers that label timings ask. */
int orv_gemm_kernel_name(int M, int N, int K, int epilogue, char* buf, int len);
/* The same for a call with packed operands (orv_gemm_t.a_packed / c_packed); an error when no kernel takes the combination (the caller then
 * keeps the row-major path). */
int orv_gemm_kernel_name_packed(int M, int N, int K, int epilogue, int a_packed, int c_packed, char* buf, int len);
/* Developer switch (sweeps, same-process A/B, per-instantiation tests): pin the tile candidate (kernel family `ring`: 0 simple,
 * 1 ring, 2 phased, 3 t8; tile bm x bn) for all later orv_gemm_bf16 calls of this process; bm = 0 returns to the cost model.
 * Same effect as the environment variable ORV_GEMM_TILE="ring,bm,bn" read at the first call. */
int orv_gemm_force_tile(int ring, int bm, int bn);
/* Number of orv_gemm_force_tile calls so far: a host-side plan derived from orv_gemm_kernel_name(_packed) (which GEMMs of a block take packed
 * operands) is valid for the epoch it was made in and is re-derived when this moves. */
int orv_gemm_force_epoch(void);
/* C[M, N] (+)= A[K, M]^T . W[K, N] - both operands row-major over the CONTRACTION index (K rows): the weight gradient dW = dY^T X of a linear
 * layer straight from the row-major dY [tokens, out] and X [tokens, in], without transposed copies (torch autograd of nn.Linear inside
 * `accelerator.backward(loss)`, train_cogvideox_control_to_video_sft.py:1093; the linears of cogvideox_control.py:232-234, 263, 439-440).
 * bf16 operands, fp32 accumulation, bf16 C; accumulate != 0 adds to C (gradient accumulation).  M % 8 == 0, N % 192 == 0 or N % 256 == 0. */
int orv_gemm_tn_bf16(const void* A, long lda, const void* W, long ldw, void* C, long ldc, int M, int N, int K, int accumulate, void* stream);
/* C[P, Q] (+)= alpha * U[M, P]^T . V[M, Q] with min(P, Q) <= 128: the skinny sibling of orv_gemm_tn_bf16 for the weight gradients of a
 * low-rank adapter on a linear layer, y = x W^T + b + c (x A^T) B^T: dB = c dY^T T (P = out, Q = rank) and dA = dT^T X (P = rank, Q = in),
 * contracted over all M tokens (torch autograd of the adapter linears inside `accelerator.backward(loss)`,
 * train_cogvideox_control_to_video_sft.py:1093).  Both operands are row-major over the contraction index M (row strides ldu / ldv elements:
 * column slices of wider buffers are fine), bf16; accumulation is fp32.  The contraction is cut into chunks whose count and boundaries
 * depend on (M, P, Q) only; every chunk's fp32 partial goes to `scratch` (orv_gemm_tn_skinny_scratch(M, P, Q) bytes, 16-byte aligned), the
 * partials are added in chunk order, scaled by alpha, the old C is added in fp32 when accumulate != 0, and the sum is rounded to bf16 once.
 * No atomics: two runs give identical bits.  P % 16 == 0, Q % 16 == 0, M >= 1, ldu / ldv / ldc multiples of 8, 16-byte aligned pointers. */
long orv_gemm_tn_skinny_scratch(int M, int P, int Q);
int orv_gemm_tn_skinny_bf16(const void* U, long ldu, const void* V, long ldv, void* C, long ldc, int M, int P, int Q, float alpha,
                            int accumulate, void* scratch, void* stream);

/* -- MXFP8 inference GEMMs (opt-in: CogVideoXTransformer3DModelTraj.enable_mxfp8) ------------------------------------------------- */
/* Format (OCP MX, e4m3fn elements): a row-major [rows, K] bf16 matrix (K % 32 == 0) is cut into blocks of 32 consecutive K elements;
 * block j of row r is 32 e4m3fn bytes q[r, 32j .. 32j+31] plus one e8m0 scale byte s[r, j] (value 2^(s - 127)).  q is [rows, K] uint8,
 * s [rows, K / 32] uint8, both row-major and dense.  The scale is 2^e with e the smallest integer such that amax / 2^e <= 448 (amax =
 * the block's largest |x|), clamped to [-127, 127]; amax == 0 gives e = 0 (byte 0x7F).  Element = x / 2^e rounded to nearest-even in
 * e4m3fn, saturated to +-448 (-0 stays -0: byte 0x80).  The input of every producer is the bf16 value, so a fused producer and "bf16,
 * then orv_mxfp8_quantize" give identical bytes.  Weights [N, K] use the same rule along K. */
/* q, s = MXFP8 of x [M, K] bf16 (row stride ldx elements, 16-byte aligned rows); any M, K % 32 == 0. */
int orv_mxfp8_quantize(const void* x, long ldx, void* q, void* s, int M, int K, void* stream);
/* C = epilogue(A . W^T + bias) with A = g->A (e4m3 [M, K], row stride g->lda bytes) scaled by a_scale [M, K / 32] and W = g->W (e4m3
 * [N, K], row stride g->ldw bytes) scaled by w_scale [N, K / 32]; fp32 accumulation on the block-scaled MFMA (the scales enter as the
 * MFMA's scale operands), bf16 C.  Epilogues 0, 1 and 2 and the R / gate / grp / cmap fields as orv_gemm_bf16; no Y, no packed layouts,
 * no epilogue 3 / 4.  No split-K: every output element is one fixed accumulation over K, whatever M.  K % 128 == 0, N % 128 == 0,
 * lda / ldw multiples of 16 (16-byte aligned rows). */
int orv_gemm_mxfp8(const orv_gemm_t* g, const void* a_scale, const void* w_scale, void* stream);
/* orv_layernorm_modulate with its bf16-rounded output written as MXFP8: q [batch * seq, D] (row stride D bytes), s [batch * seq, D / 32].
 * Byte-identical to orv_layernorm_modulate followed by orv_mxfp8_quantize (the same kernel and arithmetic; quantised at the store).
 * D % 32 == 0.  Feeds the QKV and FFN1 GEMMs of the MXFP8 mode (cogvideox_control.py:232-234, 439). */
int orv_layernorm_modulate_mxfp8(const void* x, int ldx, orv_rowmap_t xmap, void* q, void* s, const void* gamma, const void* beta,
                                 const float* scale, const float* shift, long mod_b, long mod_g, orv_groups_t grp, int batch, int D,
                                 float eps, void* stream);

/* -- backward (training) ------------------------------------------------------------------------------ */
/* dst[c, r] = src[r, c] ([R, C] bf16 -> [C, ld_dst], columns [R, ld_dst) zero-filled).  Feeds the NT GEMM with the
 * K-contiguous operands of dgrad (W^T) and wgrad (dY^T, X^T): dX = dY . W, dW = dY^T . X (torch autograd of nn.Linear). */
int orv_transpose_bf16(const void* src, int ld_src, void* dst, int ld_dst, int R, int C, void* stream);
/* orv_transpose_bf16 with colsum[c] += sum_r src[r, c] taken in the same pass (fp32 atomics): dY^T for the weight gradient and the
 * bias gradient of one nn.Linear from ONE read of dY (orv_transpose_bf16 followed by orv_colsum reads it twice). */
int orv_transpose_colsum_bf16(const void* src, int ld_src, void* dst, int ld_dst, int R, int C, float* colsum, void* stream);
/* out[c] += sum_r src[r, c] (fp32 atomics): bias gradients. */
int orv_colsum(const void* src, int ld, float* out, int R, int C, void* stream);
/* Adjoint of out = x + gate[b,g(row)] * y (cogvideox_control.py:419-421,442-443): dy = gate * dout (bf16),
 * dgate[b,g,:] += sum_rows dout * y (table laid out like `gate`; per-workgroup partials in `scratch`, then reduced). */
long orv_gated_residual_bwd_scratch(orv_groups_t grp, int batch, int D);   /* floats of per-workgroup partial sums */
int orv_gated_residual_bwd(const void* dout, const void* y, const float* gate, float* dgate, void* dy, float* scratch,
                           long mod_b, long mod_g, orv_groups_t grp, int batch, int D, void* stream);
/* Adjoint of orv_layernorm_modulate: dx[xmap(r)] = LN-path gradient (+ dres[xmap(r)] if given), and fp32 sums
 * dscale/dshift (tables like scale/shift, +=), dgamma/dbeta [D] (+=): per-workgroup partial column sums go to `scratch`
 * (orv_layernorm_modulate_bwd_scratch() floats) and are reduced by two small kernels.  Any output may be NULL. */
long orv_layernorm_modulate_bwd_scratch(orv_groups_t grp, int batch, int D);
int orv_layernorm_modulate_bwd(const void* dy, const void* x, orv_rowmap_t xmap, const void* dres, void* dx,
                               const void* gamma, const void* beta, const float* scale, float* dscale, float* dshift,
                               float* dgamma, float* dbeta, float* scratch, long mod_b, long mod_g, orv_groups_t grp,
                               int batch, int D, float eps, void* stream);
/* Adjoint of orv_modulation_tables for all n_tab AdaLN linears at once (cogvideox_control.py:117-130,:172 under autograd):
 * dtab fp32 [n_tab, B, 1+T, width] (d out); cond_v bf16 [B*T, E] = SiLU(temb + action_emb) rows, cond_t bf16 [B, E] =
 * SiLU(temb); W device array of n_tab weight pointers as in the forward.  Writes gW bf16 [n_tab, width*(1+text), E]
 * and gb fp32 [n_tab, width*(1+text)] (overwritten), accumulates d_cond_v fp32 [B*T, E] / d_cond_t fp32 [B, E].
 * Rows are processed 32 at a time (one pass over the weights up to B*T = 32). */
int orv_modulation_tables_bwd(const float* dtab, const void* cond_v, const void* cond_t, const void* const* W, void* gW,
                              float* gb, float* d_cond_v, float* d_cond_t, int n_tab, int B, int T, int E, int width,
                              int text, void* stream);
/* Small-row (R <= 4096) linear adjoint for the conditioning MLPs / AdaLN linears: dW[N,K] (+)= dy^T x (bf16),
 * db[N] (+)= colsum(dy) (fp32), dx[R,K] += dy W (fp32 atomics).  dy fp32 [R, ldy].  Any of dW/dx may be NULL. */
int orv_small_linear_bwd(const float* dy, int ldy, const void* x, int ldx, const void* W, void* dW, float* db, float* dx,
                         int lddx, int R, int N, int K, int accumulate, void* stream);
/* Fused AdamW step on bf16 params/grads with fp32 moments (torch.optim.AdamW semantics, base_train.yaml:143-153);
 * `clip_coef` (device scalar or NULL) multiplies the gradient (global-norm clipping, train...sft.py:1095-1100). */
int orv_adamw(void* p, const void* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps,
              float weight_decay, int step, const float* clip_coef, void* stream);
/* The same AdamW update over ONE flat buffer (every parameter a segment padded to 2048 elements; seg_start[nseg] int64
 * element offsets and seg_active[nseg] bytes on the device): one launch per optimizer step instead of one per parameter.
 * Segments with seg_active == 0 (no gradient this step) are left untouched, as torch.optim.AdamW does. */
int orv_adamw_flat(void* p, const void* g, float* m, float* v, long n, const long* seg_start,
                   const unsigned char* seg_active, int nseg, float lr, float beta1, float beta2, float eps,
                   float weight_decay, int step, const float* clip_coef, void* stream);
/* Same, with ONE STEP COUNT PER SEGMENT (seg_step[nseg] int32 on the device, the count INCLUDING this update; NULL = the
 * global `step`): torch.optim.AdamW keeps `state[p]["step"]` per parameter, so a parameter that was skipped in earlier
 * steps (no gradient) gets the bias correction of its own count. */
int orv_adamw_flat_steps(void* p, const void* g, float* m, float* v, long n, const long* seg_start,
                         const unsigned char* seg_active, const int* seg_step, int nseg, float lr, float beta1, float beta2,
                         float eps, float weight_decay, int step, const float* clip_coef, void* stream);
/* orv_adamw_flat_steps with an opt-in parameter precision (FusedAdamW(param_precision=...)):
 *   mode 0 "bf16"       - exactly orv_adamw_flat_steps (the same kernel); `lo` and `seed` are ignored.
 *   mode 1 "split_fp32" - an exact fp32 master weight in 2 extra bytes per element: `lo` (int16[n], same layout as p) holds the low
 *                         half, master_bits = (p_bits << 16) + sign_extend(lo); the update runs on the master and writes back
 *                         p_bits = (master_bits + 0x8000) >> 16 (nearest, ties AWAY from zero), lo = master_bits - (p_bits << 16).
 *                         A non-finite master writes the matching non-finite bf16 (NaN quiet) and lo = 0.  `lo` is required.
 *   mode 2 "stochastic" - the fp32 result is stored as p_bits = (bits + r) >> 16, r a uniform 16-bit integer from a counter-based
 *                         hash of (seed, step, flat element index) only (defined in orv_amd/csrc/optim.hip): identical on every
 *                         run and every data-parallel rank.  Non-finite results are written unperturbed; a finite result is never
 *                         carried into infinity (largest finite bf16 instead).  `lo` is ignored.
 * Any other mode, or mode 1 without `lo`, returns non-zero with an orv_last_error message. */
int orv_adamw_flat_ex(void* p, const void* g, float* m, float* v, long n, const long* seg_start,
                      const unsigned char* seg_active, const int* seg_step, int nseg, float lr, float beta1, float beta2,
                      float eps, float weight_decay, int step, const float* clip_coef, void* lo, int mode, unsigned seed,
                      void* stream);
/* orv_adamw_flat_ex with the two moments kept as block-scaled fp8 (FusedAdamW(state_precision="fp8"); the format is
 * defined bit for bit in orv_amd/csrc/optim_s8.hip): m8 / v8 uint8[n] hold the first moment as e4m3fn and the second as e5m2 bytes in the
 * flat layout of p, m_exp / v_exp uint8[n / 256] one scale byte e + 127 per block of 256 elements.  The update dequantises the old
 * moments, runs the fp32 formula of orv_adamw_flat_ex with the second moment floored in the denominator at the smallest positive value
 * of its block's incoming grid (2^(e_v_old - 16)), stores the weight by `mode` and the new moments stochastically rounded with offsets
 * from a hash of (seed, step, flat index) only.  Inactive segments keep every byte. */
int orv_adamw_flat_s8(void* p, const void* g, unsigned char* m8, unsigned char* v8, unsigned char* m_exp, unsigned char* v_exp, long n,
                      const long* seg_start, const unsigned char* seg_active, const int* seg_step, int nseg, float lr, float beta1,
                      float beta2, float eps, float weight_decay, int step, const float* clip_coef, void* lo, int mode, unsigned seed,
                      void* stream);          /* mode 0 / 1 / 2 as orv_adamw_flat_ex; mode 0 here = nearest-even bf16 */
/* Parameter groups on the flat layout (FusedAdamW(param groups)).  seg_group[nseg] (device bytes) names the group of
 * every segment; the table of the groups' two numbers travels BY VALUE with the launch, so a schedule changes any group's rate at every
 * step with no host-to-device copy and no device table to keep in sync.  Every seg_group value must be < ngroups (the caller builds the
 * table and checks it there; the kernels leave a segment whose byte is >= 8 untouched). */
#define ORV_ADAMW_MAX_GROUPS 8
typedef struct {
    int ngroups;                                  /* 1..ORV_ADAMW_MAX_GROUPS */
    float lr[ORV_ADAMW_MAX_GROUPS];
    float weight_decay[ORV_ADAMW_MAX_GROUPS];
} orv_adamw_groups_t;
/* orv_adamw_flat_ex / orv_adamw_flat_s8 with the scalars lr and weight_decay replaced by (seg_group, groups): a segment's update is exactly
 * the parent's formula, in the same operation order (the same device function), with its group's two numbers - the group is looked up once
 * per workgroup, which never straddles a segment.  All three modes; inactive segments keep every byte.  A null buffer, ngroups outside
 * 1..8 or n % 2048 != 0 return non-zero with an orv_last_error message before anything is launched.
 * orv_adamw_flat_s8_groups has one argument more, common_count: the per-segment count that most segments are at (<= 0: `step`).  The fp8
 * kernel takes the host's bias corrections for a segment whose count equals it and works out its own (two powf per lane, a third more
 * kernel time) for any other; `step` seeds the rounding and keeps advancing over a skipped step, the counts do not, so after a skip the
 * caller passes the count they stopped at.  The result does not depend on it. */
int orv_adamw_flat_groups(void* p, const void* g, float* m, float* v, long n, const long* seg_start, const unsigned char* seg_active,
                          const int* seg_step, int nseg, const unsigned char* seg_group, orv_adamw_groups_t groups, float beta1,
                          float beta2, float eps, int step, const float* clip_coef, void* lo, int mode, unsigned seed, void* stream);
int orv_adamw_flat_s8_groups(void* p, const void* g, unsigned char* m8, unsigned char* v8, unsigned char* m_exp, unsigned char* v_exp,
                             long n, const long* seg_start, const unsigned char* seg_active, const int* seg_step, int nseg,
                             const unsigned char* seg_group, orv_adamw_groups_t groups, float beta1, float beta2, float eps, int step,
                             int common_count, const float* clip_coef, void* lo, int mode, unsigned seed, void* stream);
/* out[i] = sum of g^2 over segment i = elements [seg_start[i], seg_start[i + 1]) of the bf16 buffer g (seg_start int64[nseg + 1] on the
 * device, multiples of 8), in fp64, for all nseg segments in ONE launch, one workgroup per segment, no atomics.  The order of the
 * additions is fixed by the segment's length alone (stated in orv_amd/csrc/optim_groups.hip; restated in numpy in
 * tests/adamw_groups_ref.py): two runs give the same bits, and a non-finite element makes its own segment's sum non-finite and nothing
 * else. */
int orv_segment_sumsq(const void* g, const long* seg_start, int nseg, double* out, void* stream);
#define ORV_GUARD_REPORT 11      /* doubles in `report`: [0] ss, [1..8] one sum per group, [9] running skip count, [10] skipped (0 / 1) */
/* The decisions of one optimizer step, on the device, in one launch of one workgroup (operation order in optim_groups.hip):
 *   ss = seg_ss[0] + seg_ss[1] + ... in index order (fp64); report[1 + j] the same over the segments of group j;
 *   *clip_coef = fp32(c * inv_world), c = max_grad_norm / (sqrt(ss) * inv_world + 1e-6) where that is below 1, else 1 (a NaN stays a NaN;
 *                max_grad_norm == 0: c = 1, no clipping), all in fp64;
 *   skip_nonfinite != 0 and ss not finite: every byte of seg_active is cleared, report[9] += 1, report[10] = 1 and *clip_coef = 0;
 *   otherwise report[10] = 0.  report[9] is read and written, so the caller zeroes `report` once. */
int orv_step_guard(const double* seg_ss, const unsigned char* seg_group, int nseg, float max_grad_norm, float inv_world,
                   int skip_nonfinite, unsigned char* seg_active, float* clip_coef, double* report, void* stream);
/* x fp32[n] -> exactly the bytes orv_adamw_flat_s8 would store for the fp32 moments x at that (seed, step, flat index), and back
 * (exact).  format 0 = first moment (e4m3fn), 1 = second moment (e5m2); n % 256 == 0. */
int orv_state8_quantize(const float* x, unsigned char* q, unsigned char* exps, long n, int format, unsigned seed, int step, void* stream);
int orv_state8_dequantize(const unsigned char* q, const unsigned char* exps, float* x, long n, int format, void* stream);
/* Fused Prodigy (FusedProdigy; the rule and its operation order are stated in orv_amd/csrc/optim_prodigy.hip) on the flat
 * layout of orv_adamw_flat_ex mode 1: p bf16[n] + lo int16[n] are the split fp32 master, g bf16[>= n] the gradient, m / v / s fp32[n] the
 * per-element state, p0 bf16[n] the weight at a parameter's first update, seg_start / seg_active / seg_step as in orv_adamw_flat_ex
 * (seg_step REQUIRED: a segment whose count is 1 captures p0 = the bf16 part of its master).  One step is these three calls on one stream;
 * no scalar leaves the device.  state is fp64[8] on the device: d, d_max, d_numerator, d_denom, d_hat, k (completed updates), the dlr of
 * the running step, the skip flag; a fresh optimizer holds {d0, d0, 0, 0, 0, 0, 0, 0}.
 *   orv_prodigy_moments    - updates m, v, s of the active segments from the OLD d and k (dlr = d lr bc is computed in the kernel) and stores
 *                            one fp64 pair per 2048-element chunk, partials[2 c] = sum (d / d0) dlr g (p0 - w), partials[2 c + 1] = sum |s|
 *                            (zeros for the chunks of an inactive segment).  No atomics: the result depends on the inputs only.
 *   orv_prodigy_recurrence - one workgroup adds the nchunks pairs in fp64 and advances d, d_max, d_numerator, d_hat, k; when the denominator
 *                            is 0 (nothing ever had a non-zero gradient) it leaves them as they are and raises the skip flag.
 *   orv_prodigy_update     - w -= (wd dlr) w (decoupled decay) ; w -= dlr m / (sqrt(v) + d eps) on the master with the NEW d, stored by the
 *                            rounding rule of orv_adamw_flat_ex mode 1; does nothing when the skip flag is set.
 * Inactive segments keep every byte of p, lo, m, v, s and p0.  n % 2048 != 0, eps <= 0, d0 <= 0 or a null buffer (clip_coef may be NULL)
 * return non-zero with an orv_last_error message before anything is launched. */
int orv_prodigy_moments(const void* p, const void* lo, const void* g, void* p0, float* m, float* v, float* s, long n,
                        const long* seg_start, const unsigned char* seg_active, const int* seg_step, int nseg, const double* state,
                        double* partials, float lr, float beta1, float beta2, float beta3, float weight_decay, int decouple,
                        int safeguard_warmup, int use_bias_correction, double d0, const float* clip_coef, void* stream);
int orv_prodigy_recurrence(double* state, const double* partials, long nchunks, float lr, float beta1, float beta2, float beta3,
                           int use_bias_correction, double d0, double d_coef, double growth_rate, void* stream);
int orv_prodigy_update(void* p, void* lo, const float* m, const float* v, long n, const long* seg_start,
                       const unsigned char* seg_active, int nseg, const double* state, float eps, float weight_decay, int decouple,
                       void* stream);
/* Fused CAME (FusedCAME): Adam with a factored second moment and a confidence term, on the flat layout of
 * orv_adamw_flat_ex.  Operation order, g the gradient times *clip_coef (NULL: 1), every state value fp32 and zero at the start:
 *      q = g g + eps1
 *      segment of shape [B, R, C] (R > 0), per matrix:   r = b2 r + (1-b2) mean_j q ;  c = b2 c + (1-b2) mean_i q
 *                                                        u = (g rsqrt(r_i / mean_i r)) rsqrt(c_j)
 *      unfactored segment (R == 0):                      v = b2 v + (1-b2) q ;  u = g rsqrt(v)
 *      k = max(1, sqrt(mean of u u over the segment) / clip_threshold) ;  u = u / k
 *      m = b1 m + (1-b1) u ;  s = (u - m)^2 + eps2                                      (the new m)
 *      factored:   res_r = b3 res_r + (1-b3) mean_j s ;  res_c = b3 res_c + (1-b3) mean_i s
 *                  out = (m rsqrt(res_r_i / mean_i res_r)) rsqrt(res_c_j) ;      unfactored:   out = m
 *      w = w - (weight_decay lr) w  (weight_decay != 0) ;  w = w - lr out
 * w and its store are those of orv_adamw_flat_ex: mode 0 the bf16 weight rounded to nearest-even, mode 1 the split fp32 master p + lo.
 * geom is a DEVICE table of 12 int64 per segment: B, R, C, first tile, first matrix, offset of the segment in r / res_r, in c / res_c, in v
 * (a multiple of 2048), in the row partial sums, in the column partial sums, element count, 0.  A factored segment owns B matrices, B R
 * rows, B C columns, B ceil(R / 64) ceil(C / 256) tiles, B R ceil(C / 256) row partials and B C ceil(R / 64) column partials; an unfactored
 * one ceil(numel / 2048) tiles and as many elements of v, padded to 2048; n_tiles .. n_colp are the totals.  scratch (fp32, contents
 * meaningless between steps, every value read in a step is written in it first) holds at least
 * n_rowp + n_colp + n_tiles + n_rows + n_cols + 2 nseg values; its last 2 nseg are (k, RMS of u) per segment after a step.
 * One step is the launches which = 0 .. 6 in order on one stream (orv_came_step issues them all): no host read, no atomics, every sum in a
 * fixed order.  Inactive segments and padding keep every byte.  A null descriptor or buffer, n % 2048 != 0, a mode other than 0 / 1,
 * eps1 <= 0, clip_threshold <= 0 or a scratch that is too small return non-zero with an orv_last_error message before anything is launched. */
typedef struct {
    void* p; void* lo; const void* g; float* m;                  /* bf16[n], int16[n] (mode 1) or NULL, bf16[>= n], fp32[n] */
    float* r; float* c; float* res_r; float* res_c; float* v;    /* fp32[n_rows], [n_cols], [n_rows], [n_cols], [n_v] */
    long n, n_rows, n_cols, n_v;
    const long* seg_start; const unsigned char* seg_active; int nseg;
    const long* geom; long n_tiles, n_mats, n_rowp, n_colp;
    float* scratch; long n_scratch;
    const float* clip_coef;
    float lr, beta1, beta2, beta3, eps1, eps2, clip_threshold, weight_decay;
    int mode;
} orv_came_t;
int orv_came_launch(const orv_came_t* d, int which, void* stream);
int orv_came_step(const orv_came_t* d, void* stream);
/* Exponential moving average of the weights on the flat layout of orv_adamw_flat_ex (orv_amd.FusedEMA; defined bit for
 * bit in orv_amd/csrc/optim_ema.hip).  shadow fp32[n] lies in the segment layout of p bf16[n]; lo int16[n] (NULL where the optimizer
 * keeps none) holds the low halves of the fp32 masters.
 *   orv_ema_update  - shadow <- shadow - one_minus_decay * (shadow - theta), three separately rounded fp32 operations in that order;
 *                     theta is the master (p_bits << 16) + sign_extend(lo) where lo is given, fp32(p) otherwise.  Padding stays +0.
 *   orv_ema_swap_in - stash_p <- p and stash_lo <- lo (each may be NULL: not kept), then p <- the nearest-even bf16 of shadow (NaN quiet);
 *                     zero_lo != 0 also clears lo, so that the master equals the written value.  One launch.
 * Workgroups of 2048 elements, 16-byte accesses, no atomics.  A null required buffer, n % 2048 != 0, a buffer that is not 16-byte
 * aligned, one_minus_decay outside [0, 1], or stash_lo / zero_lo without lo return non-zero with an orv_last_error message before
 * anything is launched. */
int orv_ema_update(float* shadow, const void* p, const void* lo, long n, float one_minus_decay, void* stream);
int orv_ema_swap_in(void* p, void* lo, const float* shadow, void* stash_p, void* stash_lo, long n, int zero_lo, void* stream);
/* dst_ptr[s][j] = bf16(src[src_off[s] + j]), j < len[s], for nseg segments (src_off / dst_ptr / len are DEVICE arrays; dst_ptr holds
 * device addresses of bf16 storage; max_len = max len[s]): the small fp32-accumulated parameter gradients go from the backward's
 * accumulator arena into the fused optimizer's flat gradient buffer in one launch (the reference leaves this to autograd's
 * per-parameter accumulation, train_cogvideox_control_to_video_sft.py:1093). */
int orv_scatter_f32_to_bf16(const float* src, const long* src_off, const long* dst_ptr, const int* len, int nseg, int max_len,
                            void* stream);
/* out[0] += sum g^2 (gradient-norm reduction, orv/utils.py:166-174). */
int orv_sumsq(const void* g, long n, float* out, void* stream);

/* src[B*S, ld] columns [col0 + h*64, +64) -> dst[b,h,d,pos(s)] per head (pos = s with bits 2<->3 exchanged, zero for
 * s >= S): the forward's V^T when the qk LayerNorm rides in the QKV GEMM (epilogue 4), and the sequence-contiguous copies
 * (q'^T, k^T, dO^T) the attention backward contracts over. */
int orv_head_transpose(const void* src, int ld, int col0, void* dst, int B, int S, int H, int s_pad, void* stream);
/* Adjoint of orv_attention_fwd on the fused path (q pre-multiplied by scale*log2 e in orv_qkv_prep): given out, dout and
 * the saved lse, writes dqkv[B*S, ld_dqkv] = (dq | dk | dv) w.r.t. the normalised, un-premultiplied q, k and v.
 * qT/kT/doT: orv_head_transpose of q', k, dout.  neg_lse2/neg_delta: fp32 scratch [B,H,s_pad]. */
int orv_attention_bwd(const void* qkv, int ld_qkv, const void* qT, const void* kT, const void* out, const void* dout,
                      int ld_out, const void* doT, const float* lse, float* neg_lse2, float* neg_delta, void* dqkv,
                      int ld_dqkv, int B, int S, int H, int s_pad, float scale, void* stream);
/* Adjoint of orv_qkv_prep for the q and k thirds, in place on dqkv: inverse RoPE, LayerNorm(64) backward (qkv_raw = the
 * QKV GEMM output before orv_qkv_prep); dgq/dbq/dgk/dbk fp32 [64] accumulate the norm_q / norm_k parameter gradients. */
int orv_qkv_prep_bwd(const void* qkv_raw, void* dqkv, const void* gq, const void* gk, const float* rope_cos,
                     const float* rope_sin, float* dgq, float* dbq, float* dgk, float* dbk, float* scratch, int B, int S,
                     int H, int n_text, float eps, void* stream);   /* scratch: fp32 [ceil(S/64)*H*B*256] */

/* -- attention -------------------------------------------------------------------------------- */
/* Non-causal, unmasked softmax(q k^T * scale) v over the joint text+video sequence, head_dim 64
 * (F.scaled_dot_product_attention at cogvideox_control.py:256-258).  q,k are read in place from the packed qkv
 * buffer [B*S, ld_qkv] (q at column h*64, k at column H*64 + h*64); vT [B,H,64,s_pad] from orv_qkv_prep / orv_head_transpose;
 * out [B*S, H*64] bf16 (heads merged as :260); lse fp32 [B,H,S] or NULL (log-sum-exp, natural log, for backward). */
int orv_attention_fwd(const void* qkv, int ld_qkv, const void* vT, void* out, int ld_out, float* lse, int B, int S,
                      int H, int s_pad, float scale, void* stream);
/* The same attention (V read in place) when the caller can BOUND the scores: |q . k| * scale * log2(e) <= score_bound for every
 * (query, key) of the call.  ORV always applies the per-head qk LayerNorm (cogvideox_control.py:243-247), so the bound follows
 * from norm_q / norm_k's affine parameters alone.  With the fused scale (q pre-multiplied) and score_bound <= 90 (16-byte aligned
 * output; <= 60 otherwise) the softmax runs WITHOUT a running max or rescale (P = exp2(s) stays a normal fp32 / bf16 number);
 * otherwise identical to orv_attention_fwd.  lse as there. */
int orv_attention_fwd_bounded(const void* qkv, int ld_qkv, void* out, int ld_out, float* lse, int B, int S, int H, float scale,
                              float score_bound, void* stream);
/* orv_attention_fwd_bounded writing `out` in the packed P16 layout (orv_gemm_t: orv_packed_rows(B S) x (H 64) bf16, 16-byte aligned) - the A
 * operand of the attention out-projection (cogvideox_control.py:263) without a row-major copy.  Needs scale * log2(e) == 1 (q pre-multiplied)
 * and 0 < score_bound <= orv_attention_static_limit(1): the caller checks and otherwise uses the row-major entry points. */
int orv_attention_fwd_packed(const void* qkv, int ld_qkv, void* out, float* lse, int B, int S, int H, float scale, float score_bound,
                             void* stream);
/* orv_attention_fwd_bounded with a workspace: at shapes whose grid ends in a small extra round of workgroups (the headline shape:
 * 1560 workgroups on 512 slots) the items of that round are cut into key ranges whose unnormalised partial results meet in `ws`
 * (fixed summation order: deterministic).  ws >= orv_attention_ws_bytes(B, S, H) bytes, 256-byte aligned, reusable across calls on one
 * stream; ws == NULL or an unsplit shape (ws_bytes 0): exactly orv_attention_fwd_bounded. */
size_t orv_attention_ws_bytes(int B, int S, int H);
int orv_attention_fwd_bounded_ws(const void* qkv, int ld_qkv, void* out, int ld_out, float* lse, int B, int S, int H, float scale,
                                 float score_bound, void* ws, size_t ws_bytes, void* stream);
/* Largest score_bound for which orv_attention_fwd_bounded(_dev) runs the fixed-shift softmax (16-byte aligned out: 90; else 60). */
float orv_attention_static_limit(int aligned_out);
/* orv_attention_fwd_bounded with the bound as ONE fp32 in device memory (the training step recomputes the per-layer bounds on the
 * device after every optimizer update, train_cogvideox_control_to_video_sft.py:1095-1104: no device -> host read per step).  Both
 * softmax forms are launched; the workgroups of the one the scalar does not select exit at once. */
int orv_attention_fwd_bounded_dev(const void* qkv, int ld_qkv, void* out, int ld_out, float* lse, int B, int S, int H, float scale,
                                  const float* score_bound_dev, void* stream);
/* Developer switch, in the manner of orv_gemm_kernel_name: the kernel symbol(s) a forward-attention entry point launches for a call, spelled
 * as in the source (two launches: joined by " + ").  Host arithmetic only, no GPU work.  entry: 0 orv_attention_fwd without vT, 1 with
 * vT, 2 _bounded, 3 _packed, 4 _bounded_dev; aligned_out: ld_out % 8 == 0 and a 16-byte aligned out.  The opt-in key split of _bounded_ws
 * depends on the caller's workspace and is not reported. */
int orv_attention_kernel_name(int entry, int B, int S, int H, float scale, float score_bound, int aligned_out, char* buf, int len);

/* -- T5 text encoder (orv_amd.t5.T5EncoderModel) ------------------------------------------------------------------------------------ */
/* The reference encodes prompts with transformers' T5EncoderModel, `text_encoder(ids)[0]` (orv/models/text_encoder.py:34, called from
 * the pipeline at orv/models/cogvideox_control.py:1290-1299).  These three kernels are what that encoder (T5 v1.1: RMS LayerNorm, unscaled
 * attention with a relative-position bias, gated-GELU FFN, no biases) needs beside orv_gather_rows (the embedding) and orv_gemm_bf16 (the
 * projections; the residual adds are its epilogue 2 with R == C).  All three validate before any launch, never allocate, use no atomics
 * (two runs are bit-identical) and are stream-ordered. */
/* out[b, i, h, :] = sum_j softmax_j(q_i . k_j + bias_rel[h, j - i + S - 1]) v_j: T5 self-attention (transformers T5Attention.forward as
 * reached from orv/models/text_encoder.py:34 and cogvideox_control.py:1290-1299): NO 1/sqrt(d) scale, the bias added in fp32 before the
 * row maximum, the true row maximum subtracted (scores are unbounded), no key mask (the reference passes no attention_mask).  qkv
 * [B S, ld_qkv] bf16 packed as orv_attention_fwd reads it (q at column h*64, k at H*64 + h*64, v at 2*H*64 + h*64; head_dim 64); bias_rel
 * fp32 [H, 2S - 1], entry j - i + S - 1 = the bias of query i and key j; out [B S, ld_out] bf16, columns [0, H*64) of rows [0, B S)
 * written and nothing else.  fp32 accumulation on the MFMA.  1 <= S <= orv_t5_attention_max_seq() (512: one head's K and V stay in one
 * workgroup's LDS); a longer S is an error that names the maximum.  ld_qkv, ld_out multiples of 8, 16-byte aligned pointers. */
int orv_t5_attention_max_seq(void);
int orv_t5_attention_fwd(const void* qkv, int ld_qkv, const float* bias_rel, void* out, int ld_out, int B, int S, int H, void* stream);
/* y[m, :] = w * bf16(x[m, :] * rsqrt(mean(x[m, :]^2) + eps)): transformers T5LayerNorm.forward (no mean subtraction, no bias; statistics
 * in fp32, the normalised row rounded to bf16 before the gain as there) - every layer_norm / final_layer_norm of the encoder behind
 * orv/models/text_encoder.py:34 and cogvideox_control.py:1290-1299.  x, y [M, D] bf16 (row strides ldx / ldy, multiples of 8), w [D]
 * bf16; D % 64 == 0; x == y is allowed. */
int orv_t5_rmsnorm(const void* x, int ldx, const void* w, void* y, int ldy, int M, int D, float eps, void* stream);
/* out[m, f] = gelu_tanh(h[m, f]) * h[m, F + f], fp32, rounded to bf16 once: the gate of transformers T5DenseGatedActDense
 * ("gated-gelu": gelu_new(wi_0 x) * wi_1 x) inside the encoder of orv/models/text_encoder.py:34 / cogvideox_control.py:1290-1299, with
 * both wi projections coming from ONE orv_gemm_bf16 over the stacked weight [2 d_ff, d_model].  h [M, 2F] bf16 (row stride ldh), out
 * [M, F] bf16 (row stride ldo); F % 8 == 0, strides multiples of 8. */
int orv_geglu(const void* h, int ldh, void* out, int ldo, int M, int F, void* stream);

/* -- sampler ---------------------------------------------------------------------------------- */
/* One fused scheduler update on n elements (cogvideox_control.py:1433-1459 + diffusers
 * CogVideoXDDIMScheduler.step / CogVideoXDPMScheduler.step, v-prediction):
 *   v    = guidance ? v_u + guidance_scale * (v_c - v_u) : v_c            (CFG, :1440-1443)
 *   x0   = sa * x - sb * v
 *   d    = old_x0 ? m3 * x0 - m4 * old_x0 : x0
 *   x'   = cx * x + cd * d + cn * noise                                   (noise may be NULL when cn == 0)
 * x, x' bf16 (the pipeline's latents dtype); v_c/v_u bf16 model outputs; x0_out/old_x0 fp32; noise fp32.
 * DDIM: cx = a_t, cd = b_t, cn = 0.  DPM: cx = m1, cd = -m2, cn = m_noise. Coefficients are computed on the host in
 * float64 (orv_amd/schedulers.py) exactly as the reference does. */
int orv_sched_step(const void* x, const void* v_c, const void* v_u, float guidance_scale, const float* old_x0,
                   const float* noise, void* x_out, float* x0_out, float sa, float sb, float m3, float m4, float cx,
                   float cd, float cn, long n, void* stream);

/* mean + exp(0.5*clamp(logvar,-30,20)) * eps, times `scale` (diffusers DiagonalGaussianDistribution.sample used at
 * cogvideox_control.py:1173-1177,1334-1358; train_cogvideox_control_to_video_sft.py:890-898) with the
 * [B,2C,F,H,W] -> [B,F,C,H,W] permute fused.  moments bf16, eps fp32 [B,C,F,H,W], out bf16. */
int orv_gaussian_sample(const void* moments, const float* eps, void* out, int B, int C, int F, int HW, float scale,
                        void* stream);

/* -- VAE: AutoencoderKLCogVideoX decode / encode, reference call sites
 *    orv/models/cogvideox_control.py:1476-1479 (decode_latents) and :1161-1166 (vae.encode of the reference frame); the
 *    arithmetic is diffusers' (absent: parity unpinned, oracle/vae.py).  Activations are channels-last bf16 [B,T,H,W,C]. -- */
/* Patch matrix of a causal 3-D / per-frame 2-D convolution for orv_gemm_bf16: dst[mc, Kpad] rows for voxels [m0, m0+mc) of the
 * [B*T*H*W] output grid, column = tap * C + channel (tap = (dt*kh + dy)*kw + dx), tail columns zero.  Folded into the gather:
 * replicate-first-frame temporal padding (CogVideoXCausalConv3d), zero spatial padding (pad_lo in front), spatial stride 1|2,
 * nearest x2 upsampling of the source in H,W (ups_s) and in T (ups_t: 1 = every frame doubled, 2 = first frame kept).
 * t_shift = frames of temporal context the caller prepended to src (the conv_cache diffusers carries from one frame batch to
 * the next): output frame t reads source frames t + t_shift - (kt-1) + dt; with 0 the first frame is replicated instead. */
int orv_vae_im2col(const void* src, void* dst, int B, int Ts, int Hs, int Ws, int C, int T, int H, int W, int kt, int kh, int kw,
                   int stride, int pad_lo, int ups_s, int ups_t, int t_shift, int Kpad, long m0, long mc, void* stream);
/* The same convolution as ONE launch, without the patch matrix (implicit GEMM): the GEMM's A operand is gathered by the LDS-DMA
 * from the channels-last source (geometry fields as orv_vae_im2col's), W = packed weights [N, taps*C] (column = tap*C + ci),
 * epilogue 0 (bias) or 2 (R + acc + bias: the resnet's residual add).  g->A is ignored; g->M = B*T*H*W, g->K = taps*C.
 * Requires C % 64 == 0 (one 64-deep K-tile = 64 channels of one tap). */
typedef struct {
    const void* src;
    int B, Ts, Hs, Ws, C;        /* source [B, Ts, Hs, Ws, C] bf16 */
    int T, H, W;                 /* output voxel grid */
    int kt, kh, kw, stride, pad_lo, ups_s, ups_t, t_shift;
} orv_conv_t;
int orv_conv_gemm_bf16(const orv_gemm_t* g, const orv_conv_t* c, void* stream);
/* GroupNorm statistics: sums[B, G, 2] = (sum, sum of squares) of x[B, N, C] per group, fp32, no atomics (bit-reproducible).
 * scratch: orv_vae_groupnorm_scratch(B, N, C, G) floats. */
long orv_vae_groupnorm_scratch(int B, long N, int C, int G);
int orv_vae_groupnorm_stats(const void* x, float* sums, float* scratch, int B, long N, int C, int G, void* stream);
/* out = act(GroupNorm(x) [* zy[z(v)] + zb[z(v)]]): affine GroupNorm from `sums`, CogVideoXSpatialNorm3D modulation by
 * conv_y(zq) / conv_b(zq) given at LATENT resolution [B,Tz,hz,wz,C] and looked up by F.interpolate(nearest) index rules
 * (first frame of an odd-length clip apart), optional SiLU.  zy == zb == NULL: plain GroupNorm.
 * out is [B, out_lead + T, H, W, C]: the first out_lead (0..8) frames of every clip are left untouched - the caller puts the
 * causal context of the NEXT convolution there (conv_cache frames or copies of the first frame; orv_conv_t.t_shift = out_lead). */
int orv_vae_norm_apply(const void* x, void* out, const float* sums, const void* gamma, const void* beta, const void* zy,
                       const void* zb, int B, int T, int H, int W, int C, int G, int Tz, int hz, int wz, float eps, int silu_act,
                       int out_lead, void* stream);
/* Seam blend of the tiled decode / encode (diffusers AutoencoderKLCogVideoX.blend_v / blend_h, enabled by the reference at
 * /root/reference/orv/pipeline/inference_control_to_video.py:98-99): channels-last tiles a [outer, Ha, Wa, C], b [outer, Hb, Wb, C]
 * bf16; in place on b: vertical (horizontal = 0): b[.., y, :] = a[.., Ha - extent + y, :] (1 - y / extent) + b[.., y, :] y / extent
 * for y < extent (Wa == Wb); horizontal: the same along x with a = the tile to the left (Ha == Hb). */
int orv_vae_blend(const void* a, void* b, int outer, int Ha, int Wa, int Hb, int Wb, int C, int extent, int horizontal,
                  void* stream);

/* -- Gaussian rasterizer: ORV's depth / semantic conditioning renders ----------------------------------------------------------------
 * Forward splatting of N 3-D Gaussians into colour [3,H,W], feature [F,H,W], depth [1,H,W] and alpha [1,H,W] planes, replacing the CUDA
 * extension orv/ops/diff-gaussian-rasterization (Python surface diff_gaussian_rasterization/__init__.py:21-236) that
 * orv/dataset/gs_render.py:97-171 calls once per frame and view from orv/dataset/prepare_dataset.py:2023-2235.  fp32 throughout,
 * forward only, no atomics (bit-reproducible).  The arithmetic contract - near plane 0.01, 16x16 tiles, the radius and tile-rectangle
 * rules, the blend thresholds 1/255 and 1e-4, the (depth, index) order - is written out in DESIGN.md section 12.  Matrices are
 * row-major [4,4] device arrays in the row-vector convention of gs_render.py:128-130: viewmatrix = (world-to-camera)^T,
 * projmatrix = viewmatrix @ P^T, a point maps as [p,1] @ M.  A render is four calls with two torch steps between them:
 *   preprocess -> cumsum(tiles_touched) -> tile_keys -> stable sort of the keys -> tile_ranges (ranges zeroed first) -> render.
 *
 * Per Gaussian (replaces the extension's preprocessing stage behind gs_render.py:151-160): view-space depth, pixel centre xy [N,2],
 * conic_opacity [N,4] = (A, B, C, opacity), radii [N] (0 = invisible), rect [N,4] = (x0, y0, x1, y1) in tiles, tiles_touched [N].
 * N = 0 launches nothing. */
int orv_gs_preprocess(const float* means3D, const float* scales, const float* rotations, const float* opacities,
                      const float* viewmatrix, const float* projmatrix, int N, int H, int W, float tanfovx, float tanfovy,
                      float scale_modifier, float* xy, float* conic_opacity, float* depth, int* radii, int* rect,
                      int* tiles_touched, void* stream);
/* One int64 key per (Gaussian, covered tile) pair (replaces the extension's key duplication stage behind gs_render.py:151-160):
 * tile id (y * ceil(W/16) + x) in the high 32 bits, the fp32 bits of the view-space depth in the low 32; gaussian_idx [L] holds the
 * Gaussian of each pair.  offsets [N] = inclusive prefix sum of tiles_touched (int64), L = offsets[N-1] < 2^31.  Pairs are laid out by
 * ascending Gaussian index, so a stable sort of the keys breaks depth ties by index.  N = 0 or L = 0 launches nothing. */
int orv_gs_tile_keys(const int* rect, const float* depth, const long* offsets, int N, int H, int W, long L, long* keys,
                     int* gaussian_idx, void* stream);
/* ranges [tiles, 2] = [start, end) of each tile's run in the sorted keys (replaces the extension's range identification stage behind
 * gs_render.py:151-160).  The caller zeroes `ranges` first: a tile no Gaussian covers keeps (0, 0).  L = 0 launches nothing. */
int orv_gs_tile_ranges(const long* sorted_keys, long L, int H, int W, int* ranges, void* stream);
/* Per-tile front-to-back blend (replaces the extension's render stage behind gs_render.py:151-160; outputs in the order of
 * diff_gaussian_rasterization/__init__.py:103): one 256-thread workgroup per tile, the tile's list point_list[start, end) staged through
 * LDS in batches of 256 entries.  colors [N,3], features [N,F] with 0 <= F <= 16 (F = 0: no feature plane, features / out_feature may
 * be NULL), bg [3] on the device.  color = sum + T * bg, feature and depth are plain sums, alpha = 1 - T.  With L = 0 the per-Gaussian
 * arrays may be NULL and every pixel is background. */
int orv_gs_render(const int* ranges, const int* point_list, long L, const float* xy, const float* conic_opacity,
                  const float* depth, const float* colors, const float* features, int N, int F, const float* bg, int H, int W,
                  float* out_color, float* out_feature, float* out_depth, float* out_alpha, void* stream);

/* -- Point-cloud voxelization: ORV's occupancy preparation --------------------------------------------------------------------------
 * Hard, dynamic and semantic voxelization of a point cloud points [N, C] (fp32, x y z first), replacing the CUDA extension orv/ops/voxelize
 * (Python surface orv/ops/voxelize/voxelization.py:42-122) that points_to_voxels (orv/dataset/prepare_dataset.py:137-198) calls for every
 * frame from get_occupancy (:887-1039).  The definition is the sequential walk of orv/ops/voxelize/voxelization_cpu.cpp:71-102; the
 * arithmetic contract - fp32 (p - lo) / vs with a correctly rounded divide, grid = round((hi - lo) / vs) in fp32, voxels in order of first
 * appearance, slots in point order, the two caps, the vote's tie rule - is written out in DESIGN.md section 13.  Integer and copied-float
 * outputs, no order-dependent atomic: bit-reproducible.  voxel size (vx, vy, vz) and range (x0, y0, z0 = min; x1, y1, z1 = max) are passed
 * by value, already rounded to fp32.  A voxelization is three or four calls with two torch steps between them:
 *   coors -> stable sort of the keys -> segments (first zeroed) -> inclusive int32 cumsum(first), M = min(last, max_voxels) -> scatter | vote.
 *
 * Cells per axis (x, y, z) by the reference's rule (voxelization_cpu.cpp:118-121, :147-150).  Host only. */
int orv_voxel_grid_size(float vx, float vy, float vz, float x0, float y0, float z0, float x1, float y1, float z1, int* grid);
/* Per point (replaces dynamic_voxelize_kernel, orv/ops/include/voxelization_kernel.cuh:9-46, in the CPU form of voxelization_cpu.cpp:7-46):
 * coors [N,3] int32 = (z, y, x) cell, or (-1, -1, -1) for a point outside the range or with a NaN / infinite coordinate; keys [N] int64 =
 * (z * gy + y) * gx + x, the largest int64 for an invalid point (keys may be NULL: dynamic voxelization needs coors only).
 * N = 0 launches nothing. */
int orv_voxel_coors(const float* points, int N, int C, float vx, float vy, float vz, float x0, float y0, float z0, float x1, float y1,
                    float z1, int* coors, long* keys, void* stream);
/* On the stably sorted keys with order [N] int64 = the point of each sorted entry (replaces point_to_voxelidx_kernel,
 * voxelization_kernel.cuh:91-132, where every point scans all earlier points): start [N] = sorted position of the entry's segment head
 * (-1 for an invalid point), seglen [N] = the segment's length at its head (0 elsewhere), first [N] (zeroed by the caller) = 1 at the
 * point that opens a voxel. */
int orv_voxel_segments(const long* sorted_keys, const long* order, int N, int* start, int* seglen, int* first, void* stream);
/* Hard voxelization's output (replaces determin_voxel_num <<<1, 1>>> and assign_point_to_voxel / assign_voxel_coors,
 * voxelization_kernel.cuh:134-163 and :48-88): csum [N] int32 = inclusive prefix sum of first, M = min(csum[N-1], max_voxels).  An entry of
 * voxel csum[first point] - 1 < M with rank < max_points copies its C features to voxels [M, max_points, C] (zeroed by the caller); the
 * head writes coors [M,3] (z, y, x) and num_points_per_voxel [M] = min(length, max_points).  N = 0 or M = 0 launches nothing. */
int orv_voxel_scatter(const float* points, const int* point_coors, const long* order, const int* start, const int* seglen,
                      const int* csum, int N, int C, int max_points, int M, float* voxels, int* coors, int* num_points_per_voxel,
                      void* stream);
/* The semantic vote fused with the scatter (replaces the torch post-processing of prepare_dataset.py:179-196 on the voxels buffer, which
 * is never built): the last feature holds label + 1 with 0 <= label < 255; out [M,4] int32 = (x, y, z, label), label = the most frequent
 * stored label among the voxel's first min(length, max_points) points, minus one, a tie going to the smallest label.  One wave per voxel.
 * head_of [M] int32 is scratch, filled with -1 by the caller.  N = 0 or M = 0 launches nothing. */
int orv_voxel_vote(const float* points, const int* point_coors, const long* order, const int* start, const int* seglen, const int* csum,
                   int N, int C, int max_points, int M, int* head_of, int* out, void* stream);

/* -- Occupancy labelling and sparse Gaussian scene preparation ------------------------------------------------------------------------
 * The two steps of ORV's conditioning chain between the voxelization above and the rasterizer: labelling a frame's surface points from
 * its 2-D label image (project_3d_to_2d, orv/dataset/prepare_dataset.py:878-884, and the labelling block of get_occupancy, :999-1008),
 * and turning a frame's occupancy rows into the Gaussians get_render splats (prepare_dataset.py:2069-2086 and :2148-2164) without any
 * buffer the size of the 400^3 grid.  The arithmetic contract is written out in DESIGN.md section 14.  The only atomics are integer ORs
 * on a flag and a bitmap, so every output is bit-reproducible.  A scene preparation is three calls with two torch steps between them:
 *   cell_keys -> stable sort of the keys -> mark_cells -> inclusive int32 cumsum(last), one host read of (bitmap, flag, count) ->
 *   write_gaussians.
 *
 * Per point (replaces project_3d_to_2d, prepare_dataset.py:878-884, and the gather and relabelling of :999-1008): P is the device pointer
 * of the row-major fp32 4 x 4 matrix intrin4 @ inverse(extrin) (rows 0 to 2 are read; it is never read on the host).  For j = 0, 1, 2
 * h_j = ((x P[j][0] + y P[j][1]) + z P[j][2]) + P[j][3] with every product and sum rounded to fp32 on its own (no fused multiply-add),
 * u = h_0 / h_2 and v = h_1 / h_2 by a correctly rounded divide, then truncated toward zero.  A point is inside when 0 <= trunc(u) < W
 * and 0 <= trunc(v) < H: u in (-1, 0) counts as column 0, a point behind the camera counts when it lands inside, a NaN or infinite u or
 * v is outside.  labels3d [N] int64 = labels2d[v][u] with 255 (and -1) -> 59 for a point inside, 0 outside.  labels2d [H, W] holds
 * label_bytes = 1 (uint8) or 4 (int32) per pixel.  N = 0 launches nothing. */
int orv_occ_project_labels(const float* points, int N, int C, const float* P, const void* labels2d, int label_bytes, int H, int W,
                           long* labels3d, void* stream);
/* Per occupancy row occ [M,4] int32 = (x, y, z, label) (replaces the two dense scatters of prepare_dataset.py:2153-2154 and :2162-2163
 * into 64 M-cell grids): keys [M] int64 = the dense linear index (x Y + y) Z + z, the largest int64 for a row outside the X x Y x Z grid,
 * which also sets state[1] (state [3] int64, zeroed by the caller: class bitmap, out-of-grid flag, spare).  M = 0 launches nothing. */
int orv_occ_cell_keys(const int* occ, int M, int X, int Y, int Z, long* keys, long* state, void* stream);
/* On the stably sorted keys with order [M] int64 = the row of each sorted entry (replaces torch.unique over the 64 M-cell grid,
 * prepare_dataset.py:2155-2157): last [M] int32 = 1 at the entry that closes its cell's segment - the cell's last row, whose label the
 * dense scatter keeps - else 0; the labels of those rows, clamped to [0, 59], are ORed into the bitmap state[0]. */
int orv_occ_mark_cells(const long* sorted_keys, const long* order, const int* occ, int M, int* last, long* state, void* stream);
/* Every attribute of the n surviving cells in ascending order of the dense index (replaces the [64 M, 12] one-hot of
 * prepare_dataset.py:2158 and the six boolean gathers of :2175 over the dense tensors of :2077-2086): csum [M] int32 = inclusive prefix
 * sum of last, n = csum[M-1]; order and occ as in mark_cells (the cell's coordinates are read from its row); classes = the bitmap, with bit 0 set by the caller when the grid has an empty cell.  Gaussian g gets
 * xyz [n,3] = (ax[x], ay[y], az[z]) from the three axis tables, rgb [n,3] = 0, feat [n,F] = the one-hot of popcount(classes below the
 * label), rot [n,4] = (1, 0, 0, 0), scale [n,3] = zscale[z] three times, opacity [n,1] = 1.  More classes than F channels is refused.
 * M = 0 or n = 0 launches nothing. */
int orv_occ_write_gaussians(const long* order, const int* occ, const int* last, const int* csum, int M, int n,
                            int X, int Y, int Z, const float* ax, const float* ay, const float* az, const float* zscale,
                            unsigned long classes, int F, float* xyz, float* rgb, float* feat, float* rot, float* scale, float* opacity,
                            void* stream);

/* -- Control encoding: rendered depth and label maps (or uint8 video frames) to the VAE encoder's input --------------------------------
 * Replaces the per-frame torchvision loop of orv/dataset/dataset.py:225-295 and :852-888 and the repeat / permute of
 * orv/dataset/encode_dataset.py:801-916, and writes what AutoencoderKLCogVideoX._channels_last(x, cpad=5) would.  The arithmetic contract
 * (DESIGN.md section 15), all fp32:
 *   plan     up to two stages of (resize to rh x rw, centre crop to ch x cw at (top, left)); stage 2 reads stage 1's cropped fp32 image.
 *            A crop larger than its input and a downscale beyond 4 x per axis and stage are refused.
 *   bilinear antialiased, per axis, n inputs -> o outputs: scale = float(n) / float(o); support = scale if scale >= 1 else 1; inv = 1 / scale
 *            if scale >= 1 else 1; c = scale * (i + 0.5); lo = max(int(c - support + 0.5), 0), hi = min(int(c + support + 0.5), n); tap j
 *            in [lo, hi) weighs max(0, 1 - |(j - c + 0.5) * inv|); the weights are summed in tap order and each is divided by the sum
 *            (correctly rounded); the output is the sum in tap order of x[j] * w[j].  Every product and sum is rounded to fp32 on its own
 *            (no FMA).  The horizontal pass comes first and is rounded to fp32, the vertical pass follows.
 *   nearest  source index min(int(floorf(i * (float(n) / float(o)))), n - 1); two stages compose their index maps; ids are painted after.
 *   post     depth: min(max(x, 0.01), 0.4) * 2.5; ids: palette[id] / 255; RGB: x / 255 before the resize, (x - 0.5) / 0.5 after the crop
 *            with ORV_COND_POST_NORMALIZE.
 * src [N, h, w] (fp32 or uint8 ids) or [N, h, w, 3] (uint8 RGB); palette fp32 [n_palette, 3] on the device (ids only; an id is validated by
 * the caller, the kernel reads no entry past the table); index int32 [n_out] on the device = the source frame of every output frame
 * (NULL: the identity; validated by the caller, an entry outside [0, N) gives a zero frame); plan = 6 host ints per stage (rh, rw, top,
 * left, ch, cw).  out: ORV_COND_OUT_NCHW fp32 [n_out, C, H, W] (C = 1 for an fp32 source, else 3) or ORV_COND_OUT_VAE bf16
 * [n_out, H, W, 8] (channels 0-2 the data, a single channel repeated three times, channels 3-7 zero; one 16-byte store per pixel), 16-byte
 * aligned.  One launch, a workgroup per 16 x 16 tile of the final image; a two-stage bilinear plan keeps the stage-1 pixels its tile
 * reaches in LDS.  No atomics: bit-reproducible.  n_out = 0 launches nothing. */
#define ORV_COND_SRC_F32 0
#define ORV_COND_SRC_IDS 1
#define ORV_COND_SRC_RGB8 2
#define ORV_COND_NEAREST 0
#define ORV_COND_BILINEAR 1
#define ORV_COND_POST_NONE 0
#define ORV_COND_POST_DEPTH 1
#define ORV_COND_POST_NORMALIZE 2
#define ORV_COND_OUT_NCHW 0
#define ORV_COND_OUT_VAE 1
int orv_cond_prepare(const void* src, int src_kind, int N, int h, int w, const float* palette, int n_palette, const int* index, int n_out,
                     const int* plan, int n_stage, int interp, int post, void* out, int out_kind, void* stream);

/* -- Video metrics: per-frame PSNR and SSIM of a generated clip against its ground truth, on the device ---------------------------------
 * Replaces the per-frame CPU loop of orv/pipeline/compute_metrics.py:38-80: cv2.resize(..., (320, 256), INTER_LINEAR) of both images,
 * then skimage's peak_signal_noise_ratio and structural_similarity(channel_axis=-1, data_range=1.), spread over 64 threads.  The
 * arithmetic contract.  PARITY UNPINNED: cv2 and skimage are not installed where this was written; the kernel is
 * held to this contract, and the contract's SSIM to scipy.ndimage.uniform_filter in fp64 (the filter skimage calls).
 *   source   fp32 is taken as it is; uint8 is (float)v / 255.0f (the reference's astype(float32) / 255.).
 *   resize   per axis, n inputs -> o outputs (cv2's INTER_LINEAR for float images, restated from memory): scale = 1.0 / ((double)o /
 *            (double)n); f = (float)(((double)i + 0.5) * scale - 0.5); s = floor(f); wt = f - (float)s; s < 0 gives s = 0, wt = 0;
 *            s >= n - 1 gives s = n - 1, wt = 0; the second tap is min(s + 1, n - 1).  The horizontal pass comes first,
 *            r = p[s] * (1.0f - wt) + p[s + 1] * wt, then the vertical pass over the two r rows in the same form; every product and sum is
 *            rounded to fp32 on its own (no FMA).  o == n reproduces the source exactly: the supported way to skip the resize.
 *   box mean 7 x 7: seven horizontal terms summed left to right in fp32, seven of those sums top to bottom, divided by 49.0f.
 *   SSIM     skimage's defaults (win_size 7, uniform window, K1 = 0.01, K2 = 0.03, sample covariance), per channel, with the box means
 *            ux, uy, uxx, uyy, uxy of a, b, a*a, b*b, a*b: cn = (float)(49.0 / 48.0); vx = cn * (uxx - ux * ux); vy likewise;
 *            vxy = cn * (uxy - ux * uy); C1 = (float)((0.01 R)^2), C2 = (float)((0.03 R)^2) with R = data_range;
 *            S = ((2 ux uy + C1) * (2 vxy + C2)) / ((ux ux + uy uy + C1) * (vx + vy + C2)), products and sums left to right as written,
 *            the division correctly rounded.  S is averaged in fp64 over the pixels at distance >= 3 from every border (skimage's crop)
 *            per channel; ssim = ((m0 + m1) + m2) / 3 of the three channel means.
 *   PSNR     difference and square in fp32, sum in fp64; mse = sse / (3 h w); psnr = 10 log10(R^2 / mse) in fp64, inf when mse == 0.
 * pred and gt each describe N frames of 3 channels by a device pointer, an element offset, element strides for (n, y, x, c), the number
 * of elements of the buffer behind the pointer (every element the kernel can read is checked to lie inside it) and their own source
 * height and width: uint8 or fp32 [N,H,W,3], fp32 [N,3,H,W] and width slices of either need no copy.  Both are resized to h x w (h, w
 * >= 7).  out fp64 [3, N] = mse, psnr, ssim; ssim_map fp32 [N, h - 6, w - 6, 3] or NULL; workspace = orv_frame_metrics_workspace(N, h, w)
 * bytes, 8-byte aligned, for one record of four fp64 sums per (frame, 32 x 32 tile).  Two launches: a workgroup per tile and frame keeps
 * the resized block and its 3-pixel halo in LDS (the resized images never go to HBM), then one wave per frame sums the records in a fixed
 * order.  No atomics on floating-point data: bit-reproducible.  N = 0 launches nothing. */
#define ORV_METRICS_SRC_F32 0
#define ORV_METRICS_SRC_U8 1
typedef struct {
    const void* data;      /* device pointer of the buffer */
    int kind;              /* ORV_METRICS_SRC_* */
    int h, w;              /* source height and width */
    long extent;           /* elements in the buffer behind data */
    long offset;           /* element offset of pixel (0, 0, 0, 0) */
    long stride[4];        /* element strides of (n, y, x, c) */
} orv_frames_t;
long orv_frame_metrics_workspace(int N, int h, int w);
int orv_frame_metrics(const orv_frames_t* pred, const orv_frames_t* gt, int N, int h, int w, double data_range, double* out,
                      float* ssim_map, void* workspace, long workspace_bytes, void* stream);

/* -- Point-cloud cleaning and normals: the front of ORV's reconstruction stage -----------------------------------------------------------
 * Replaces the per-frame CPU work of get_dense_points (orv/dataset/prepare_dataset.py:786-875) between the .ply points and NKSR's two
 * input tensors (:754-755): _preprocess_points (:806-822: z < 0.6, then Open3D's remove_statistical_outlier(30, 1.5)) and
 * process_nksr._preprocess_point_cloud (:729-741: estimate_normals(KDTreeSearchParamKNN(20)), orient_normals_towards_camera_location()).
 * The arithmetic contract.  PARITY UNPINNED: Open3D is not installed where this was written and has no ROCm path;
 * its semantics are restated from memory and the kernels are held to this restatement.
 *   points   fp32 [N, 3], contiguous; every distance is fp64 on the fp32 values widened exactly.
 *   kNN      d2(i, j) = (dx dx + dy dy) + dz dz with dx = (double)p_j.x - (double)p_i.x ..., every product and sum rounded to fp64 on its
 *            own (no FMA).  The neighbours of i are the k' = min(k, N) points of smallest (d2, index), in that order; i itself is a
 *            candidate at d2 = 0; a tie in d2 goes to the smaller index.  1 <= k <= 64.  idx int32 [N, k'], d2 fp64 [N, k'], ascending.
 *   outliers avg_i = (sum over the ranks, in rank order, of sqrt(d2[i, r])) / k'.  Over the V points with avg_i > 0: mean = sum / V,
 *            std = sqrt(sum (avg_i - mean)^2 / (V - 1)), thr = mean + std_ratio std; i is kept iff avg_i > 0 and avg_i < thr.  V == 0
 *            makes mean NaN and V == 1 makes std NaN: both keep nothing.  Both sums in a fixed two-stage order.
 *   normals  k' < 3 gives (0, 0, 1).  Else m = the neighbours' mean (fp64, rank order), C = sum (p - m)(p - m)^T / k' (the centred
 *            two-pass form), the normal a unit eigenvector of C's smallest eigenvalue (analytic, fp64); C == 0 gives (0, 0, 1); for a
 *            rank-1 C with line direction u the normal is e x u normalised, e the coordinate axis of the smallest |u| component.  Then
 *            v = camera - p and the normal is negated when (n.x v.x + n.y v.y) + n.z v.z < 0.  One rounding to fp32, at the store.
 * A search is four calls around one torch step: cells -> stable sort of the keys -> cell_table -> knn -> knn_brute on the queries knn
 * flagged.  The grid is (x0, y0, z0) + cell * [0, gx) x [0, gy) x [0, gz), at most 2^24 cells; cell coordinates floor((p - lo) / cell) in
 * fp64 are clamped to it, so the result does not depend on the grid - only the time does.  No atomics: bit-reproducible.  Every entry
 * point validates its arguments before any launch; N = 0 launches nothing.
 *
 * Per point, the key (z gy + y) gx + x of its clamped cell (replaces the KD-tree build of :737 and of remove_statistical_outlier, :819). */
int orv_pc_cells(const float* points, int N, float x0, float y0, float z0, double cell, int gx, int gy, int gz, long* keys, void* stream);
/* On the stably sorted keys with order [N] int64 = the point of each sorted entry (the rest of the KD-tree build, :737, :819):
 * start int32 [n_cells + 1] = the first sorted position of every cell (start[n_cells] = N), sorted_points fp32 [N, 3] = the points in
 * sorted order, so that a cell's points are contiguous. */
int orv_pc_cell_table(const long* sorted_keys, const long* order, const float* points, int N, int n_cells, int* start, float* sorted_points,
                      void* stream);
/* The k-nearest-neighbour search (replaces the KD-tree queries behind remove_statistical_outlier, :819, and KDTreeSearchParamKNN, :737).
 * One wave per query with the running list one entry per lane; the cubes of cells of ring 0..3 around the query's cell are walked until
 * the list is full and its last d2 is below the squared distance to every face of the cube that is not on the grid's border.  Rows of
 * finished queries are written to idx / d2 [N, k']; pending uint8 [N] = 1 for the others, which orv_pc_knn_brute must finish. */
int orv_pc_knn(const float* sorted_points, const long* order, const int* start, int N, int k, float x0, float y0, float z0, double cell,
               int gx, int gy, int gz, int* idx, double* d2, unsigned char* pending, void* stream);
/* The same search (:819, :737) for the Q listed queries (int64 point numbers) by a scan of all N points, one workgroup per query: what
 * keeps the result exact for every input and every cell edge. */
int orv_pc_knn_brute(const float* points, int N, int k, const long* queries, int Q, int* idx, double* d2, void* stream);
/* Statistical outlier removal on the search's d2 [N, k'] (replaces remove_statistical_outlier(nb_neighbors=30, std_ratio=1.5), :819):
 * avg fp64 [N], stats fp64 [4] = mean, std, thr, V, keep uint8 [N]; workspace = orv_pc_outlier_workspace(N) bytes, 8-byte aligned.  Six
 * launches: avg, then twice (partial sums per 1024 points, one workgroup summing the partials in order), then the mask. */
long orv_pc_outlier_workspace(int N);
int orv_pc_outlier(const double* d2, int N, int k, double std_ratio, double* avg, double* stats, unsigned char* keep, void* workspace,
                   long workspace_bytes, void* stream);
/* Normals from the search's idx [N, k'] (replaces estimate_normals(KDTreeSearchParamKNN(20)) and
 * orient_normals_towards_camera_location(), :737-738): normals fp32 [N, 3], oriented towards the camera location.  One thread per point. */
int orv_pc_normals(const float* points, const int* idx, int N, int k, double camx, double camy, double camz, float* normals, void* stream);
/* The standalone orientation (orient_normals_towards_camera_location(), :738) of given normals [N, 3] into out [N, 3], in fp64: a zero
 * normal becomes (camera - p) / |camera - p|, or (0, 0, 1) when that is zero too; any other is negated when n . (camera - p) < 0. */
int orv_pc_orient(const float* points, const float* normals, int N, double camx, double camy, double camz, float* out, void* stream);

/* -- Label-map compositing: segmentation masks to the 2-D label image and its colour preview ---------------------------------------------
 * Replaces the last non-network step of ORV's label preparation, _postprocess_labels (orv/dataset/prepare_dataset.py:1377-1486), which
 * copies [n, H, W] booleans to the host, writes them to disk, reloads them in a 16-process pool and runs 2 n boolean-index stores per
 * frame.  The contract is written out in DESIGN.md section 18.  PARITY UNPINNED for the two supervision definitions (area as the count of
 * set pixels, mask_to_xyxy as the inclusive bounding box, zeros for an empty mask): supervision is not installed where this was written.
 *   masks    F x n planes of H x W pixels, 1 <= H, W < 65536, behind one device pointer; plane (f, j) starts at element f stride_f +
 *            j stride_n (any non-negative element strides below 2^40: a permuted or sliced view needs no copy) and is contiguous.
 *            mask_bytes = 1: bool or uint8, a pixel is set where the byte is nonzero; the pointer may be any byte address.
 *            mask_bytes = 4: fp32 logits, 4-byte aligned, a pixel is set where x > threshold in IEEE terms, decided on the bits so that
 *            the device's denormal mode has no say: +-0 and NaN are not above 0, the smallest denormal and +inf are; a NaN threshold
 *            sets nothing.
 * Nothing outside a plane is read: a row or group that is not 16-byte aligned, and the last partial group, are read element by element.
 * Every value is an integer and there are no atomics: bit-reproducible.  Every argument is checked before any launch and no device
 * pointer is followed; F = 0 or n = 0 launches nothing that reads a mask.
 *
 * Per (frame, mask) plane (replaces sv.mask_to_xyxy and detections.area, prepare_dataset.py:1406-1420, and for logits the threshold of
 * :1275-1279): area int64 [F, n] = the count of set pixels, xyxy int64 [F, n, 4] = x_min, y_min, x_max, y_max, inclusive, over the set
 * pixels, all zeros for an empty mask.  bands in [1, H] row bands per plane, a workgroup each, write one record of five int32 to
 * workspace int32 [F n bands 5] (the caller's; no initial value is needed); a second launch combines a plane's records in band order. */
int orv_lm_mask_stats(const void* masks, int mask_bytes, int F, int n, int H, int W, long stride_f, long stride_n, float threshold,
                      int bands, int* workspace, long* area, long* xyxy, void* stream);
/* Per frame (replaces the two paint loops of prepare_dataset.py:1412-1444; the threshold of :1275-1279 for logits): index uint8 [F, H, W]
 * starts at 255 and color uint8 [F, H, W, 3] at 0; for k = 0 .. m - 1 in sequence, where mask j = order[k] is set, index = label_ids[j] and
 * color = palette[label_ids[j] % 60].  A pixel painted with id 255 is painted and gets its colour: the kernel carries a painted flag per
 * pixel and never tests index == 255.  order int [m] (m <= n, entries in [0, n), expected distinct; a repeated entry repaints), label_ids
 * uint8 [n] and palette uint8 [60, 3] (written in the order given: the caller arranges b, g, r) are HOST arrays, read during the call;
 * steps uint32 [m + 256] is the caller's device scratch, which the call fills stream-ordered with the paint steps and the id -> triple
 * table.  index and color are 16-byte aligned.  One lane owns 16 consecutive pixels; traffic is F m H W mask_bytes read and 4 F H W
 * written.  F = 0 launches nothing. */
int orv_lm_compose(const void* masks, int mask_bytes, int F, int n, int H, int W, long stride_f, long stride_n, float threshold,
                   const int* order, int m, const unsigned char* label_ids, const unsigned char* palette, unsigned* steps,
                   unsigned char* index, unsigned char* color, void* stream);

/* -- Cascaded rollouts: the chunk boundary on the device -----------------------------------------------------------------------------------
 * Replaces what the reference's cascade (orv/pipeline/evaluation_control_to_video.py:349-362) does on the host between two denoise loops:
 * VideoProcessor.postprocess_video(..., 'pil') (an fp32 copy of the clip to the host, two numpy passes, PIL frames) and, for the frame
 * handed to the next chunk, VideoProcessor.preprocess (PIL -> numpy -> tensor -> device).  The contract is DESIGN.md section 19.  No atomics,
 * no LDS; every output value depends on one input value: bit-reproducible.  Every argument is checked before any launch, no device pointer
 * is followed on the host, and every element a kernel can touch is checked to lie inside the extents given.
 *
 * The decoder's output to uint8 frames (replaces postprocess_video's 'pil' branch, evaluation_control_to_video.py:349): src is bf16
 * (src_bytes = 2) or fp32 (4) [B, 3, F, H, W] with element strides src_stride[5] = (b, c, f, y, x) behind a pointer to element (0, 0, 0, 0,
 * 0) with src_extent elements behind it.  Frames [f0, f1) of every clip are written to dst, uint8 [.., H, W, 3] frames of contiguous
 * rows, frame f of clip b at byte b dst_stride_b + (dst_f0 + f - f0) dst_stride_f, with dst_extent bytes behind dst: a chunk's stitched
 * range lands in the episode buffer directly.  Per value, in fp32 with one rounding per step: y = fl(fl(x / 2) + 0.5), clamped to
 * [0, 1], u = rint_half_even(fl(y * 255)); +inf gives 255, -inf 0 and NaN 0 (numpy's cast of a NaN is platform-defined).  No fast-math.
 * A lane owns 8 consecutive pixels of a row (three 16-byte plane loads for bf16, 24 output bytes as six dwords) where x is the unit
 * stride, the three plane rows are 16-byte and the destination row 4-byte aligned; the last W % 8 pixels and every other row go pixel by
 * pixel.  Traffic: 3 src_bytes + 3 bytes per pixel.  f0 == f1 launches nothing. */
int orv_frames_quantize(const void* src, int src_bytes, long src_extent, const long* src_stride, int B, int H, int W, int f0, int f1,
                        unsigned char* dst, long dst_extent, long dst_stride_b, long dst_stride_f, int dst_f0, void* stream);
/* One uint8 frame per clip to the VAE encoder's input (replaces preprocess on the PIL frame videos[0][index] and the copy to the device,
 * evaluation_control_to_video.py:361-362 and :317 into cogvideox_control.py:1366): src uint8 [B, F, H, W, 3] with byte strides
 * src_stride[5] = (b, f, y, x, c) and src_extent bytes behind it; frame `frame` of every clip goes to out bf16 [B, 1, H, W, 8], contiguous
 * and 16-byte aligned, channels 0-2 = table[u], channels 3-7 zero.  table is bf16 [256] on the device, built on the host with preprocess'
 * own statements (level / 255 in fp32, 2 x - 1 in fp32, rounded to bf16), so the values equal the host path's by construction.  A lane owns
 * a pixel: three bytes in, one 16-byte store. */
int orv_frames_handoff(const unsigned char* src, long src_extent, const long* src_stride, int B, int F, int H, int W, int frame,
                       const void* table, void* out, void* stream);

/* -- First-block step cache of the denoise loop (opt-in, lossy) ----------------------------------------------------------------------------
 * The contract is DESIGN.md section 20; the rule is restated from memory of diffusers' FirstBlockCache / ParaAttention's FBCache and is
 * not pinned against either.  x is the joint bf16 buffer [B, S = Nt + Nv, D] with row stride D; only the video rows Nt .. S - 1 of every
 * clip take part.  e, p, f, c, t are dense bf16 [B, Nv, D].  D is a multiple of 64, every tensor pointer 16-byte aligned.  Symbols: E the
 * video rows after the embedding stage, F after iteration 0 of the block loop, X after the last iteration, p the stored first residual, t
 * the stored tail residual.  Every argument is checked before any launch and no device pointer is followed on the host.  Streaming
 * kernels, 16-byte accesses, plain vector stores, no atomics: two runs give the same bits.
 *
 * Doubles of caller scratch orv_step_cache_probe needs for (B, Nv, D): two per workgroup; -1 with orv_last_error() for a bad shape. */
long orv_step_cache_scratch(int B, int Nv, int D);
/* x holds F in its video rows, e holds E.  Writes f = F (a dense copy, the same bits), c = bf16_rne(fp32(F) - fp32(E)) (one fp32
 * subtraction, one rounding) and sums fp64 [B, 2]: sums[b][0] = num_b = sum |fp32(c) - fp32(p)| and sums[b][1] = den_b = sum |fp32(p)|
 * over the clip's Nv D values; each difference is rounded once to fp32, its absolute value widened to fp64 and added in fp64, in an
 * order fixed by (Nv, D).  A NaN among the values read makes the sum it enters NaN.  scratch (n_scratch doubles, at least
 * orv_step_cache_scratch) needs no initial value: every word read is written first.  Two launches (partial sums per workgroup, then
 * one wave per clip).  Traffic: 5 B Nv D 2 bytes. */
int orv_step_cache_probe(const void* x, const void* e, const void* p, void* f, void* c, double* scratch, long n_scratch, double* sums, int B,
                         int Nt, int Nv, int D, void* stream);
/* x holds X in its video rows.  Writes t = bf16_rne(fp32(X) - fp32(f)) and p = c (the commit of the probe's residual, fused in: no
 * separate copy, no pointer swap).  Traffic: 5 B Nv D 2 bytes. */
int orv_step_cache_store(const void* x, const void* f, const void* c, void* t, void* p, int B, int Nt, int Nv, int D, void* stream);
/* The video rows of x become bf16_rne(fp32(x) + fp32(t)), in place; the text rows are not touched.  Traffic: 3 B Nv D 2 bytes. */
int orv_step_cache_apply(void* x, const void* t, int B, int Nt, int Nv, int D, void* stream);

/* -- Training-state snapshot with a checksum per tensor (orv_amd.train_state) ------------------------------------------
 * The checksum of a buffer of `bytes` bytes, all arithmetic mod 2^64: pad the bytes with zero bytes to a multiple of 4, read them as
 * little-endian u32 words w_0 .. w_{W-1}; s1 = sum w_i, s2 = sum (i + 1) w_i; an empty buffer gives (0, 0).  Bytes 01 00 00 00 02 00 00 00 03
 * are the words 1, 2, 3: s1 = 6, s2 = 14.
 *
 * One table entry: `bytes` bytes at src, copied to dst (NULL: summed only).  src and dst are 4-byte aligned, independently at any
 * residue mod 16; bytes is any count >= 0; the two ranges of an entry do not overlap.  Nothing is written outside [dst, dst + bytes). */
typedef struct {
    const void* src;
    void* dst;
    long bytes;
} orv_snapshot_entry_t;
/* The chunk size of the kernels: an entry is processed in pieces of this many bytes of its own range. */
int orv_snapshot_chunk_bytes(void);
/* Bytes of caller scratch that suffice for any table of n entries holding total_bytes bytes in all (16 per chunk, at most one partly
 * filled chunk per entry); -1 with orv_last_error() for a bad argument. */
long orv_snapshot_scratch_bytes(int n, long total_bytes);
/* Copies every entry and writes sums u64 [n][2] = (s1, s2) per entry.  `entries` is the DEVICE table the kernels read; `entries_host` holds
 * the same n entries in host memory: every pointer and count is checked there before any launch, no device pointer is followed on the
 * host, and a table the two copies disagree on is the caller's error (the kernels stay inside the table and the scratch either way).
 * Refused with ORV_EINVAL and a message, without a launch: a null table, n outside 1 .. 2^20, a null or unaligned sums, a null src with
 * bytes > 0, a src or dst that is not 4-byte aligned, overlapping ranges, a scratch that is null, not 16-byte aligned or smaller than
 * 16 bytes per chunk of this table.  Two launches for the whole table, whatever n is: one pass over the data (16-byte accesses, plain
 * vector stores, one pair of partial sums per chunk into scratch) and one combine pass (one workgroup per entry); no atomics, so two
 * runs give the same bits, and scratch needs no initial value.  Traffic: 2 x bytes for a copied entry, 1 x for a summed one. */
int orv_snapshot(const orv_snapshot_entry_t* entries, const orv_snapshot_entry_t* entries_host, int n, unsigned long long* sums,
                 void* scratch, long scratch_bytes, void* stream);
/* The same sums with no copy: every dst of the table must be NULL (refused otherwise), nothing but sums and scratch is written. */
int orv_checksum(const orv_snapshot_entry_t* entries, const orv_snapshot_entry_t* entries_host, int n, unsigned long long* sums,
                 void* scratch, long scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ORV_MI355_H */
