"""Thin tensor-level wrappers over the C ABI (one Python function per ``orv_*`` entry point).

Every function takes CUDA(HIP) tensors, checks dtype/contiguity, passes raw device pointers and the current stream to
liborv_mi355.so and returns torch tensors that own the output memory.  torch is plumbing here (device memory + streams);
all arithmetic happens in the HIP kernels.  Nothing in this module can run on CPU tensors.
"""
from __future__ import annotations

from typing import Optional, Tuple

import ctypes
import os
import torch

from ._lib import ADAMW_MAX_GROUPS as _ADAMW_MAX_GROUPS
from ._lib import AdamwGroups, Gemm, Groups, RowMap, check, lib

BF16 = torch.bfloat16
ACT = {None: 0, "none": 0, "silu": 1, "gelu_tanh": 2}


def _stream():
    return torch.cuda.current_stream().cuda_stream


# Optional live per-launch timing (bench.py's roofline leg): when a dict is installed here, gemm/attention launches are
# bracketed by HIP events recorded on the launch stream (torch's current stream), keyed by kernel + shape.
_TIMELINE = None


def start_timeline():
    global _TIMELINE
    _TIMELINE = {}


def stop_timeline():
    """-> {key: [ms, ...]} of every bracketed launch since start_timeline()."""
    global _TIMELINE
    tl, _TIMELINE = _TIMELINE, None
    torch.cuda.synchronize()
    return {k: [a.elapsed_time(b) for a, b in v] for k, v in (tl or {}).items()}


class _timed:
    def __init__(self, key):
        self.key = key

    def __enter__(self):
        if _TIMELINE is not None:
            self.a, self.b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            self.a.record()

    def __exit__(self, *exc):
        if _TIMELINE is not None:
            self.b.record()
            _TIMELINE.setdefault(self.key, []).append((self.a, self.b))


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _need(t: torch.Tensor, dtype, name: str):
    if not t.is_cuda:
        raise RuntimeError(f"orv_amd.ops: `{name}` must live on the GPU (got {t.device}); there is no CPU path")
    if t.dtype != dtype:
        raise RuntimeError(f"orv_amd.ops: `{name}` must be {dtype} (got {t.dtype})")
    return t


def groups(seq: int, n_text: int, per_group: int) -> Groups:
    return Groups(seq, n_text, per_group)


def rowmap(rows: int = 0, bstride: int = 0, off: int = 0) -> RowMap:
    return RowMap(rows, bstride, off)


def timestep_embedding(t: torch.Tensor, dim: int, flip_sin_to_cos: bool = True, freq_shift: float = 0.0):
    t = _need(t.contiguous(), torch.float32, "t")
    out = torch.empty(t.numel(), dim, dtype=BF16, device=t.device)
    check(lib().orv_timestep_embedding(_p(t), _p(out), t.numel(), dim, int(flip_sin_to_cos), float(freq_shift),
                                       _stream()), "orv_timestep_embedding")
    return out


def skinny_linear(x, W, bias=None, xb=None, xb_rep=1, act_in=None, act_out=None, out=None, out_f32=False, ldo=None,
                  omap: Optional[RowMap] = None):
    """out[m] = act_out(W . act_in(x[m] + xb[m // xb_rep]) + bias);  x [M,K] bf16, W [N,K] bf16."""
    x = _need(x.contiguous(), BF16, "x")
    W = _need(W.contiguous(), BF16, "W")
    M, K = x.shape
    N = W.shape[0]
    assert W.shape[1] == K
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32 if out_f32 else BF16, device=x.device)
        ldo = N
    check(lib().orv_skinny_linear(_p(x), _p(xb), xb_rep, _p(W), _p(bias), _p(out), M, N, K, ACT[act_in], ACT[act_out],
                                  int(out.dtype == torch.float32), ldo, omap or RowMap(0, 0, 0), _stream()),
          "orv_skinny_linear")
    return out


def patchify(src0, src1=None, p: int = 2, pt: Optional[int] = None):
    src0 = _need(src0.contiguous(), BF16, "src0")
    B, T, c0, H, W = src0.shape
    c1 = 0
    if src1 is not None:
        src1 = _need(src1.contiguous(), BF16, "src1")
        c1 = src1.shape[2]
    ptt = pt or 1
    tok = torch.empty(B, (T // ptt) * (H // p) * (W // p), (c0 + c1) * ptt * p * p, dtype=BF16, device=src0.device)
    check(lib().orv_patchify(_p(src0), c0, _p(src1), c1, _p(tok), B, T, H, W, p, pt or 0, _stream()), "orv_patchify")
    return tok


def unpatchify(x, B, T, C, H, W, p: int = 2, pt: Optional[int] = None):
    x = _need(x.contiguous(), BF16, "x")
    out = torch.empty(B, T, C, H, W, dtype=BF16, device=x.device)
    check(lib().orv_unpatchify(_p(x), _p(out), B, T, C, H, W, p, pt or 0, _stream()), "orv_unpatchify")
    return out


def gather_rows(src, idx, dst, R, D, ld_src=None, ld_dst=None):
    check(lib().orv_gather_rows(_p(src), ld_src or D, _p(idx), _p(dst), ld_dst or D, R, D, _stream()), "orv_gather_rows")
    return dst


def scatter_gated_rows(y, idx, gate, gate_b, x, R, D, seq, n_text, ldy=None, ldx=None):
    check(lib().orv_scatter_gated_rows(_p(y), ldy or D, _p(idx), _p(gate), gate_b, _p(x), ldx or D, R, D, seq, n_text,
                                       _stream()), "orv_scatter_gated_rows")
    return x


def add_rows(a, amap: Optional[RowMap], b, out, col_off, M, D, lda=None, ldb=None, ldo=None):
    _need(a, BF16, "a"), _need(b, BF16, "b"), _need(out, BF16, "out")
    check(lib().orv_add_rows(_p(a), lda or D, amap or RowMap(0, 0, 0), _p(b), ldb or D, _p(out), ldo or D, col_off, M, D,
                             _stream()), "orv_add_rows")
    return out


def layernorm_modulate(x, y, gamma, beta, scale, shift, mod_b, mod_g, grp: Groups, batch, D, eps, ldx=None, ldy=None,
                       xmap: Optional[RowMap] = None, out_packed=False):
    """``out_packed``: ``y`` is a packed P16 buffer [packed_rows(batch * seq), D] (``orv_layernorm_modulate_packed``)."""
    _need(x, BF16, "x"), _need(y, BF16, "y")
    if out_packed:
        check(lib().orv_layernorm_modulate_packed(_p(x), ldx or D, _p(y), _p(gamma), _p(beta), _p(scale), _p(shift), mod_b, mod_g, grp,
                                                  batch, D, float(eps), _stream()), "orv_layernorm_modulate_packed")
        return y
    check(lib().orv_layernorm_modulate(_p(x), ldx or D, xmap or RowMap(0, 0, 0), _p(y), ldy or D, _p(gamma), _p(beta),
                                       _p(scale), _p(shift), mod_b, mod_g, grp, batch, D, float(eps), _stream()),
          "orv_layernorm_modulate")
    return y


def layernorm_modulate_mxfp8(x, q, s, gamma, beta, scale, shift, mod_b, mod_g, grp: Groups, batch, D, eps, ldx=None,
                             xmap: Optional[RowMap] = None):
    """``layernorm_modulate`` with the bf16-rounded output written as MXFP8: ``q`` uint8 [batch * seq, D] (e4m3fn bytes) and ``s`` uint8
    [batch * seq, D / 32] (e8m0 block scales); byte-identical to ``layernorm_modulate`` followed by ``mxfp8_quantize``."""
    _need(x, BF16, "x"), _need(q, torch.uint8, "q"), _need(s, torch.uint8, "s")
    check(lib().orv_layernorm_modulate_mxfp8(_p(x), ldx or D, xmap or RowMap(0, 0, 0), _p(q), _p(s), _p(gamma), _p(beta), _p(scale),
                                             _p(shift), mod_b, mod_g, grp, batch, D, float(eps), _stream()),
          "orv_layernorm_modulate_mxfp8")
    return q, s


def mxfp8_quantize(x, M=None, K=None, q=None, s=None, ldx=None):
    """MXFP8 of a row-major bf16 [M, K] matrix (include/orv_mi355.h "MXFP8"): -> (q uint8 [M, K], s uint8 [M, K / 32])."""
    _need(x, BF16, "x")
    M = x.shape[0] if M is None else M
    K = x.shape[-1] if K is None else K
    q = torch.empty(M, K, dtype=torch.uint8, device=x.device) if q is None else _need(q, torch.uint8, "q")
    s = torch.empty(M, K // 32, dtype=torch.uint8, device=x.device) if s is None else _need(s, torch.uint8, "s")
    check(lib().orv_mxfp8_quantize(_p(x), ldx or x.stride(0), _p(q), _p(s), M, K, _stream()), "orv_mxfp8_quantize")
    return q, s


def gemm_mxfp8(A, A_scale, W, W_scale, bias, C, M, N, K, epilogue=0, R=None, r_mod=0, gate=None, gate_b=0, gate_g=0,
               grp: Optional[Groups] = None, cmap: Optional[RowMap] = None, ldc=None, ldr=None):
    """``gemm`` on MXFP8 operands: A (uint8 [M, K]) / A_scale (uint8 [M, K / 32]) and W (uint8 [N, K]) / W_scale (uint8 [N, K / 32]) from
    ``mxfp8_quantize`` / ``layernorm_modulate_mxfp8``; bf16 C; epilogues 0 / 1 / 2 as in ``gemm``."""
    for t, n in ((A, "A"), (A_scale, "A_scale"), (W, "W"), (W_scale, "W_scale")):
        _need(t, torch.uint8, n)
    _need(C, BF16, "C")
    g = Gemm()
    g.A, g.lda, g.W, g.ldw, g.bias = _p(A), K, _p(W), K, _p(bias)
    g.C, g.ldc, g.M, g.N, g.K, g.epilogue = _p(C), ldc or N, M, N, K, epilogue
    g.R, g.ldr, g.r_mod = _p(R), ldr or N, r_mod
    g.gate, g.gate_b, g.gate_g = _p(gate), gate_b, gate_g
    g.grp = grp or Groups(0, 0, 0)
    g.cmap = cmap or RowMap(0, 0, 0)
    with _timed(("gemm_mxfp8", M, N, K, epilogue)):
        check(lib().orv_gemm_mxfp8(g, _p(A_scale), _p(W_scale), _stream()), "orv_gemm_mxfp8")
    return C


def gemm_tn(A, W, C, M, N, K, accumulate=False, lda=None, ldw=None, ldc=None):
    """C[M, N] (+)= A[K, M]^T . W[K, N]  (both operands row-major over the K contraction rows: dW = dY^T X without transposes)."""
    _need(A, BF16, "A"), _need(W, BF16, "W"), _need(C, BF16, "C")
    check(lib().orv_gemm_tn_bf16(_p(A), lda or M, _p(W), ldw or N, _p(C), ldc or N, M, N, K, int(bool(accumulate)), _stream()),
          "orv_gemm_tn_bf16")
    return C


def gemm_tn_skinny_scratch(M, P, Q) -> int:
    """Bytes of fp32 scratch ``gemm_tn_skinny`` needs for this shape."""
    return int(lib().orv_gemm_tn_skinny_scratch(int(M), int(P), int(Q)))


def gemm_tn_skinny(U, V, C, M, P, Q, alpha=1.0, accumulate=False, ldu=None, ldv=None, ldc=None, scratch=None):
    """C[P, Q] (+)= alpha * U[M, P]^T . V[M, Q], min(P, Q) <= 128 (adapter weight gradients; deterministic, split over the M rows).
    ``scratch``: a uint8 / fp32 CUDA tensor of at least ``gemm_tn_skinny_scratch(M, P, Q)`` bytes (allocated when omitted)."""
    _need(U, BF16, "U"), _need(V, BF16, "V"), _need(C, BF16, "C")
    need = gemm_tn_skinny_scratch(M, P, Q)
    if scratch is None:
        scratch = torch.empty(max(need, 16), dtype=torch.uint8, device=U.device)
    elif not scratch.is_cuda or scratch.numel() * scratch.element_size() < need:
        raise ValueError(f"gemm_tn_skinny: scratch must be a CUDA tensor of at least {need} bytes")
    check(lib().orv_gemm_tn_skinny_bf16(_p(U), ldu or P, _p(V), ldv or Q, _p(C), ldc or Q, M, P, Q, float(alpha), int(bool(accumulate)),
                                        _p(scratch), _stream()), "orv_gemm_tn_skinny_bf16")
    return C


def modulation_tables(temb, action_emb, w_ptrs, b_ptrs, n_tab, B, T, E, width, text, out=None):
    """All AdaLN tables of a forward: out fp32 [n_tab, B, 1+T, width]; w_ptrs/b_ptrs int64 device tensors of pointers."""
    _need(temb, BF16, "temb")
    if out is None:
        out = torch.zeros(n_tab, B, 1 + T, width, dtype=torch.float32, device=temb.device)
    check(lib().orv_modulation_tables(_p(temb), _p(action_emb), _p(w_ptrs), _p(b_ptrs), _p(out), n_tab, B, T, E, width,
                                      int(text), _stream()), "orv_modulation_tables")
    return out


def qkv_prep(qkv, vT, gq, bq, gk, bk, rope: Optional[Tuple[torch.Tensor, torch.Tensor]], B, S, H, n_text, s_pad, eps,
             q_premul: float = 1.0, src=None):
    """In place on ``qkv``, or (``src`` given) out of place: reads ``src``, writes q' / k' / v to ``qkv``."""
    _need(qkv, BF16, "qkv")
    if vT is not None:
        _need(vT, BF16, "vT")
    cos = sin = None
    if rope is not None:
        cos, sin = (_need(r.contiguous(), torch.float32, "rope") for r in rope)
    check(lib().orv_qkv_prep_from(_p(qkv if src is None else src), _p(qkv), _p(vT), _p(gq), _p(bq), _p(gk), _p(bk), _p(cos),
                                  _p(sin), B, S, H, n_text, s_pad, float(eps), float(q_premul), _stream()), "orv_qkv_prep")


def packed_rows(rows: int) -> int:
    """Row slots of a packed P16 buffer holding ``rows`` rows (include/orv_mi355.h ``orv_gemm_t``: rounded up to the 256-row GEMM tile)."""
    return int(lib().orv_packed_rows(int(rows)))


def pack_rows16(src, M, K, dst=None, ld_src=None):
    """Row-major ``src`` [M, K] -> packed P16 ``dst`` [packed_rows(M), K] (bit copies, padding rows zero)."""
    _need(src, BF16, "src")
    if dst is None:
        dst = torch.empty(packed_rows(M), K, dtype=BF16, device=src.device)
    check(lib().orv_pack_rows16(_p(src), ld_src or K, _p(_need(dst, BF16, "dst")), M, K, _stream()), "orv_pack_rows16")
    return dst


def unpack_rows16(src, M, K, dst=None, ld_dst=None):
    """Packed P16 ``src`` -> row-major ``dst`` [M, K]."""
    _need(src, BF16, "src")
    if dst is None:
        dst = torch.empty(M, K, dtype=BF16, device=src.device)
    check(lib().orv_unpack_rows16(_p(src), _p(_need(dst, BF16, "dst")), ld_dst or K, M, K, _stream()), "orv_unpack_rows16")
    return dst


def gemm_kernel_name(M, N, K, epilogue=0, a_packed=False, c_packed=False) -> Optional[str]:
    """Kernel symbol ``gemm`` launches for this call, or None when no kernel takes the packed-operand combination."""
    buf = ctypes.create_string_buffer(96)
    if a_packed or c_packed:
        rc = lib().orv_gemm_kernel_name_packed(M, N, K, epilogue, int(bool(a_packed)), int(bool(c_packed)), buf, 96)
        return buf.value.decode() if rc == 0 else None
    check(lib().orv_gemm_kernel_name(M, N, K, epilogue, buf, 96), "orv_gemm_kernel_name")
    return buf.value.decode()


def gemm(A, W, bias, C, M, N, K, epilogue=0, R=None, r_mod=0, gate=None, gate_b=0, gate_g=0, grp: Optional[Groups] = None,
         cmap: Optional[RowMap] = None, lda=None, ldw=None, ldc=None, ldr=None, Y=None, ldy=None, qknorm=None,
         a_packed=False, c_packed=False):
    """``qknorm`` = (gamma_q, beta_q, gamma_k, beta_k, eps, q_premul, heads) with ``epilogue=4``: the QKV projection with the
    per-head qk LayerNorm fused (no RoPE).  ``a_packed`` / ``c_packed``: A is read / C is written in the packed P16 layout
    (include/orv_mi355.h ``orv_gemm_t``; buffers of ``packed_rows(M)`` row slots)."""
    _need(A, BF16, "A"), _need(W, BF16, "W"), _need(C, BF16, "C")
    g = Gemm()
    if qknorm is not None:
        gq, bq, gk, bk, eps, premul, heads = qknorm
        g.qn_gamma_q, g.qn_beta_q, g.qn_gamma_k, g.qn_beta_k = _p(gq), _p(bq), _p(gk), _p(bk)
        g.qn_eps, g.qn_premul, g.qn_heads = float(eps), float(premul), int(heads)
    g.A, g.lda, g.W, g.ldw, g.bias = _p(A), lda or K, _p(W), ldw or K, _p(bias)
    g.C, g.ldc, g.M, g.N, g.K, g.epilogue = _p(C), ldc or N, M, N, K, epilogue
    g.R, g.ldr, g.r_mod = _p(R), ldr or N, r_mod
    g.gate, g.gate_b, g.gate_g = _p(gate), gate_b, gate_g
    g.grp = grp or Groups(0, 0, 0)
    g.cmap = cmap or RowMap(0, 0, 0)
    g.Y, g.ldy = _p(Y), ldy or N
    g.a_packed, g.c_packed = int(bool(a_packed)), int(bool(c_packed))
    with _timed(("gemm", M, N, K, epilogue) + ((int(bool(a_packed)), int(bool(c_packed))) if (a_packed or c_packed) else ())):
        check(lib().orv_gemm_bf16(g, _stream()), "orv_gemm_bf16")
    return C


def linear(x2d, W, bias=None, epilogue=0):
    """Convenience: dense [M,K] x [N,K]^T (+bias, optional GELU); pads K to a multiple of 64 for odd test shapes."""
    M, K = x2d.shape
    N = W.shape[0]
    if K % 64:
        pad = 64 - K % 64
        x2d = torch.nn.functional.pad(x2d, (0, pad))
        W = torch.nn.functional.pad(W, (0, pad))
        K += pad
    x2d, W = x2d.contiguous(), W.contiguous()
    C = torch.empty(M, N, dtype=BF16, device=x2d.device)
    return gemm(x2d, W, bias, C, M, N, K, epilogue)


def attention_ws_bytes(B, S, H):
    """Workspace bytes ``attention_fwd(..., ws=)`` wants for this shape (0: the shape's grid is not key-split)."""
    return int(lib().orv_attention_ws_bytes(int(B), int(S), int(H)))


def attention_kernel_name(entry, B, S, H, scale, score_bound=0.0, aligned_out=True) -> str:
    """Kernel symbol(s) a forward-attention entry point launches for this call (``orv_attention_kernel_name``; no GPU work).
    ``entry``: 0 ``orv_attention_fwd`` without vT, 1 with vT, 2 ``_bounded``, 3 ``_packed``, 4 ``_bounded_dev``."""
    buf = ctypes.create_string_buffer(96)
    check(lib().orv_attention_kernel_name(int(entry), int(B), int(S), int(H), float(scale), float(score_bound), int(bool(aligned_out)), buf, 96),
          "orv_attention_kernel_name")
    return buf.value.decode()


def attention_packed_ok(score_bound, scale) -> bool:
    """Can ``attention_fwd(..., out_packed=True)`` run this call?  (Only the shift-free ping-pong kernel writes the packed layout.)"""
    return (score_bound is not None and 0.0 < float(score_bound) <= float(lib().orv_attention_static_limit(1))
            and abs(float(scale) * 1.4426950408889634 - 1.0) < 1e-6
            and os.environ.get("ORV_ATTN_PP", "1") != "0" and os.environ.get("ORV_ATTN_STATIC", "1") != "0")


def attention_fwd(qkv, vT, out, B, S, H, s_pad, scale, lse=None, ld_qkv=None, ld_out=None, score_bound=None, score_bound_dev=None, ws=None,
                  out_packed=False):
    """``score_bound`` (V in place only): a guaranteed upper bound of |q . k| * scale * log2(e) over the whole call - the kernel
    then runs its fixed-shift softmax when the bound is small enough (``orv_attention_fwd_bounded``).  ``score_bound_dev``: the
    same bound as a one-element fp32 DEVICE tensor (``orv_attention_fwd_bounded_dev``: no host read; training).
    ``out_packed``: ``out`` is a packed P16 buffer [packed_rows(B S), H 64] (``orv_attention_fwd_packed``; check ``attention_packed_ok``)."""
    _need(qkv, BF16, "qkv"), _need(out, BF16, "out")
    if out_packed:
        with _timed(("attention", B, S, H)):
            check(lib().orv_attention_fwd_packed(_p(qkv), ld_qkv or 3 * H * 64, _p(out), _p(lse), B, S, H, float(scale), float(score_bound),
                                                 _stream()), "orv_attention_fwd_packed")
        return out
    if score_bound_dev is not None and vT is None:
        _need(score_bound_dev, torch.float32, "score_bound_dev")
        if score_bound_dev.numel() != 1:
            raise ValueError("attention_fwd: score_bound_dev must hold exactly one fp32 value")
        with _timed(("attention", B, S, H)):
            check(lib().orv_attention_fwd_bounded_dev(_p(qkv), ld_qkv or 3 * H * 64, _p(out), ld_out or H * 64, _p(lse), B, S, H,
                                                      float(scale), _p(score_bound_dev), _stream()), "orv_attention_fwd_bounded_dev")
        return out
    if score_bound is not None and vT is None and ws is not None:
        # key-split last round (orv_attention_fwd_bounded_ws): ws from attention_ws_bytes(B, S, H), reusable on one stream
        if ws.dtype != torch.uint8 or not ws.is_cuda:
            raise ValueError("attention_fwd: ws must be a uint8 CUDA tensor")
        with _timed(("attention", B, S, H)):
            check(lib().orv_attention_fwd_bounded_ws(_p(qkv), ld_qkv or 3 * H * 64, _p(out), ld_out or H * 64, _p(lse), B, S, H,
                                                     float(scale), float(score_bound), _p(ws), ws.numel(), _stream()),
                  "orv_attention_fwd_bounded_ws")
        return out
    if score_bound is not None and vT is None:
        with _timed(("attention", B, S, H)):
            check(lib().orv_attention_fwd_bounded(_p(qkv), ld_qkv or 3 * H * 64, _p(out), ld_out or H * 64, _p(lse), B, S, H,
                                                  float(scale), float(score_bound), _stream()), "orv_attention_fwd_bounded")
        return out
    if vT is not None:               # legacy form: pre-transposed V (attn_fwd_v1); None = V read in place (attn_fwd_v2)
        _need(vT, BF16, "vT")
    with _timed(("attention", B, S, H)):
        check(lib().orv_attention_fwd(_p(qkv), ld_qkv or 3 * H * 64, _p(vT), _p(out), ld_out or H * 64, _p(lse), B, S,
                                      H, s_pad, float(scale), _stream()), "orv_attention_fwd")
    return out


def sched_step(x, v_c, v_u, guidance_scale, old_x0, noise, sa, sb, m3, m4, cx, cd, cn, want_x0=True):
    x = _need(x.contiguous(), BF16, "x")
    v_c = _need(v_c.contiguous(), BF16, "v_c")
    if v_u is not None:
        v_u = _need(v_u.contiguous(), BF16, "v_u")
    if old_x0 is not None:
        old_x0 = _need(old_x0.contiguous(), torch.float32, "old_x0")
    if noise is not None:
        noise = _need(noise.contiguous(), torch.float32, "noise")
    for name, o in (("v_c", v_c), ("v_u", v_u), ("old_x0", old_x0), ("noise", noise)):
        if o is not None and o.numel() != x.numel():
            raise ValueError(f"sched_step: {name} has {o.numel()} elements, x has {x.numel()}")
    x_out = torch.empty_like(x)
    x0 = torch.empty(x.shape, dtype=torch.float32, device=x.device) if want_x0 else None
    check(lib().orv_sched_step(_p(x), _p(v_c), _p(v_u), float(guidance_scale), _p(old_x0), _p(noise), _p(x_out), _p(x0),
                               float(sa), float(sb), float(m3), float(m4), float(cx), float(cd), float(cn), x.numel(),
                               _stream()), "orv_sched_step")
    return x_out, x0


def gaussian_sample(moments, eps, scale):
    moments = _need(moments.contiguous(), BF16, "moments")
    eps = _need(eps.contiguous(), torch.float32, "eps")
    B, C2, F, H, W = moments.shape
    out = torch.empty(B, F, C2 // 2, H, W, dtype=BF16, device=moments.device)
    check(lib().orv_gaussian_sample(_p(moments), _p(eps), _p(out), B, C2 // 2, F, H * W, float(scale), _stream()),
          "orv_gaussian_sample")
    return out


# ---- backward (training) ----------------------------------------------------------------------------------------------
_TPAD = 64 if os.environ.get("ORV_TRANSPOSE_PAD", "128") == "64" else 128      # A/B switch: 64 = the round-1..5 padding


def transpose(src, R, C, ld_dst=None, out=None, ld_src=None, colsum=None):
    """[R, C] bf16 -> [C, ld_dst] (zero padded): K-contiguous operand for dgrad/wgrad.  ld_dst defaults to the row stride of ``out`` when
    one is given, else to R rounded up to 128 - the t8 GEMM kernels need K % 128 == 0, and a contraction padded to 64 only
    (CogVideoX1.5-5B at B = 4: 7048 tokens -> 7104) sent every weight-gradient GEMM of configs[4] to the older ring kernel (round 6:
    profiles/r6_train_5b_ckpt_kernel_stats_summary.txt, 17 % of the step in gemm_pp_kernel).
    ``colsum`` (fp32 [C], accumulated into): the column sums of ``src`` from the same pass (bias gradient beside dY^T)."""
    _need(src, BF16, "src")
    if ld_dst is None:
        ld_dst = int(out.stride(0)) if out is not None else (R + _TPAD - 1) // _TPAD * _TPAD
    if out is None:
        out = torch.empty(C, ld_dst, dtype=BF16, device=src.device)
    if colsum is not None:
        _need(colsum, torch.float32, "colsum")
        if colsum.numel() < C or not colsum.is_contiguous():
            raise ValueError(f"transpose: colsum needs {C} contiguous fp32 elements")
        if os.environ.get("ORV_TRANSPOSE_COLSUM", "1") == "0":       # A/B switch: two passes over src
            check(lib().orv_transpose_bf16(_p(src), ld_src or C, _p(out), ld_dst, R, C, _stream()), "orv_transpose_bf16")
            check(lib().orv_colsum(_p(src), ld_src or C, _p(colsum), R, C, _stream()), "orv_colsum")
            return out
        check(lib().orv_transpose_colsum_bf16(_p(src), ld_src or C, _p(out), ld_dst, R, C, _p(colsum), _stream()),
              "orv_transpose_colsum_bf16")
        return out
    check(lib().orv_transpose_bf16(_p(src), ld_src or C, _p(out), ld_dst, R, C, _stream()), "orv_transpose_bf16")
    return out


_scatter_tables = {}


def scatter_f32_to_bf16(src, segments):
    """``segments``: [(offset into ``src`` (fp32, flat), destination bf16 tensor (contiguous))] - every destination receives
    bf16(src[offset : offset + numel]) in ONE launch.  The device-side tables are cached per (offsets, destinations) list: the
    backward of a given model produces the same list every step."""
    _need(src, torch.float32, "src")
    if not segments:
        return
    for o, d in segments:                    # every call: a recycled address must not smuggle another dtype past the cached table
        _need(d, BF16, "destination")
        if not d.is_contiguous() or o < 0 or o + d.numel() > src.numel():
            raise ValueError("scatter_f32_to_bf16: destinations must be contiguous and sources inside `src`")
    key = (src.device.index, tuple((int(o), d.data_ptr(), d.numel()) for o, d in segments))
    tab = _scatter_tables.get(key)
    if tab is None:
        if len(_scatter_tables) > 16:
            _scatter_tables.clear()
        dev = src.device
        tab = (torch.tensor([k[0] for k in key[1]], dtype=torch.int64, device=dev),
               torch.tensor([k[1] for k in key[1]], dtype=torch.int64, device=dev),
               torch.tensor([k[2] for k in key[1]], dtype=torch.int32, device=dev), max(k[2] for k in key[1]))
        _scatter_tables[key] = tab
    check(lib().orv_scatter_f32_to_bf16(_p(src), _p(tab[0]), _p(tab[1]), _p(tab[2]), len(segments), tab[3], _stream()),
          "orv_scatter_f32_to_bf16")


def colsum(src, out, R, C, ld=None):
    _need(src, BF16, "src"), _need(out, torch.float32, "out")
    check(lib().orv_colsum(_p(src), ld or C, _p(out), R, C, _stream()), "orv_colsum")
    return out


def gated_residual_bwd(dout, y, gate, dgate, dy, mod_b, mod_g, grp, batch, D):
    scratch = torch.empty(lib().orv_gated_residual_bwd_scratch(grp, batch, D), dtype=torch.float32, device=dout.device)
    check(lib().orv_gated_residual_bwd(_p(dout), _p(y), _p(gate), _p(dgate), _p(dy), _p(scratch), mod_b, mod_g, grp, batch, D,
                                       _stream()), "orv_gated_residual_bwd")
    return dy


def layernorm_modulate_bwd(dy, x, dres, dx, gamma, beta, scale, dscale, dshift, dgamma, dbeta, mod_b, mod_g, grp, batch, D,
                           eps, xmap: Optional[RowMap] = None):
    scratch = None
    if dgamma is not None or dbeta is not None or scale is not None:
        scratch = torch.empty(lib().orv_layernorm_modulate_bwd_scratch(grp, batch, D), dtype=torch.float32, device=dy.device)
    check(lib().orv_layernorm_modulate_bwd(_p(dy), _p(x), xmap or RowMap(0, 0, 0), _p(dres), _p(dx), _p(gamma), _p(beta),
                                           _p(scale), _p(dscale), _p(dshift), _p(dgamma), _p(dbeta), _p(scratch), mod_b, mod_g,
                                           grp, batch, D, float(eps), _stream()), "orv_layernorm_modulate_bwd")
    return dx


def modulation_tables_bwd(dtab, cond_v, cond_t, w_ptrs, d_cond_v, d_cond_t, n_tab, B, T, E, width, text):
    """Adjoint of ``modulation_tables``: returns (gW bf16 [n_tab, width*(1+text), E], gb fp32 [n_tab, width*(1+text)])."""
    _need(dtab, torch.float32, "dtab"), _need(cond_v, BF16, "cond_v")
    ntot = width * (2 if text else 1)
    gW = torch.empty(n_tab, ntot, E, dtype=BF16, device=dtab.device)
    gb = torch.empty(n_tab, ntot, dtype=torch.float32, device=dtab.device)
    check(lib().orv_modulation_tables_bwd(_p(dtab), _p(cond_v), _p(cond_t), _p(w_ptrs), _p(gW), _p(gb), _p(d_cond_v),
                                          _p(d_cond_t), n_tab, B, T, E, width, int(text), _stream()),
          "orv_modulation_tables_bwd")
    return gW, gb


def small_linear_bwd(dy, x, W, dW, db, dx, R, N, K, accumulate=True, ldy=None, ldx=None, lddx=None):
    _need(dy, torch.float32, "dy")
    check(lib().orv_small_linear_bwd(_p(dy), ldy or N, _p(x), ldx or K, _p(W), _p(dW), _p(db), _p(dx), lddx or K, R, N, K,
                                     int(accumulate), _stream()), "orv_small_linear_bwd")


def adamw(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, clip_coef=None):
    check(lib().orv_adamw(_p(p), _p(g), _p(m), _p(v), p.numel(), float(lr), float(beta1), float(beta2), float(eps),
                          float(weight_decay), int(step), _p(clip_coef), _stream()), "orv_adamw")


def adamw_flat(p, g, m, v, seg_start, seg_active, lr, beta1, beta2, eps, weight_decay, step, clip_coef=None, seg_step=None):
    check(lib().orv_adamw_flat_steps(_p(p), _p(g), _p(m), _p(v), p.numel(), _p(seg_start), _p(seg_active), _p(seg_step),
                                     seg_active.numel(), float(lr), float(beta1), float(beta2), float(eps),
                                     float(weight_decay), int(step), _p(clip_coef), _stream()), "orv_adamw_flat_steps")


ADAMW_MODES = {"bf16": 0, "split_fp32": 1, "stochastic": 2}


def adamw_flat_ex(p, g, m, v, seg_start, seg_active, lr, beta1, beta2, eps, weight_decay, step, clip_coef=None, seg_step=None, lo=None,
                  mode=0, seed=0):
    """``adamw_flat`` with a parameter-precision mode (``ADAMW_MODES``): 0 the plain bf16 update, 1 an exact fp32 master split into the
    bf16 weight and the int16 buffer ``lo`` (same length as ``p``), 2 stochastic rounding of the fp32 result from a hash of
    (``seed``, ``step``, flat index)."""
    mode = ADAMW_MODES.get(mode, mode)
    _need(p, BF16, "p"), _need(g, BF16, "g"), _need(m, torch.float32, "m"), _need(v, torch.float32, "v")
    _need(seg_start, torch.int64, "seg_start"), _need(seg_active, torch.uint8, "seg_active")
    if seg_step is not None:
        _need(seg_step, torch.int32, "seg_step")
    if clip_coef is not None:
        _need(clip_coef, torch.float32, "clip_coef")
    if lo is not None:
        _need(lo, torch.int16, "lo")
        if lo.numel() != p.numel():
            raise RuntimeError(f"orv_amd.ops: `lo` holds {lo.numel()} elements, `p` {p.numel()}")
    for name, t in (("p", p), ("g", g), ("m", m), ("v", v), ("seg_start", seg_start), ("seg_active", seg_active), ("seg_step", seg_step),
                    ("lo", lo)):
        if t is not None and not t.is_contiguous():
            raise RuntimeError(f"orv_amd.ops: `{name}` must be contiguous")
    if g.numel() < p.numel() or m.numel() != p.numel() or v.numel() != p.numel() or seg_start.numel() != seg_active.numel() + 1:
        raise RuntimeError("orv_amd.ops: adamw_flat_ex buffers do not share one flat layout")
    check(lib().orv_adamw_flat_ex(_p(p), _p(g), _p(m), _p(v), p.numel(), _p(seg_start), _p(seg_active), _p(seg_step),
                                  seg_active.numel(), float(lr), float(beta1), float(beta2), float(eps), float(weight_decay),
                                  int(step), _p(clip_coef), _p(lo), int(mode), int(seed) & 0xFFFFFFFF, _stream()), "orv_adamw_flat_ex")


PRODIGY_STATE = ("d", "d_max", "d_numerator", "d_denom", "d_hat", "k", "dlr", "skip")      # the fp64[8] device state of orv_prodigy_*


def _need_prodigy_layout(what, p, lo, m, v, seg_start, seg_active, state, extra=()):
    _need(p, BF16, "p"), _need(lo, torch.int16, "lo"), _need(m, torch.float32, "m"), _need(v, torch.float32, "v")
    _need(seg_start, torch.int64, "seg_start"), _need(seg_active, torch.uint8, "seg_active"), _need(state, torch.float64, "state")
    for name, t in (("p", p), ("lo", lo), ("m", m), ("v", v), ("seg_start", seg_start), ("seg_active", seg_active), ("state", state)) + tuple(extra):
        if t is not None and not t.is_contiguous():
            raise RuntimeError(f"orv_amd.ops: `{name}` must be contiguous")
    n = p.numel()
    if (lo.numel() != n or m.numel() != n or v.numel() != n or seg_start.numel() != seg_active.numel() + 1
            or state.numel() != len(PRODIGY_STATE)):
        raise RuntimeError(f"orv_amd.ops: {what} buffers do not share one flat layout (state: fp64[{len(PRODIGY_STATE)}])")


def prodigy_moments(p, lo, g, p0, m, v, s, seg_start, seg_active, seg_step, state, partials, lr, beta1, beta2, beta3, weight_decay=0.0,
                    decouple=True, safeguard_warmup=False, use_bias_correction=False, d0=1e-6, clip_coef=None):
    """Launch 1 of a fused Prodigy step (``orv_prodigy_moments``): the moments ``m``, ``v``, ``s`` of the active segments from the OLD ``d`` and
    ``k`` in ``state`` (fp64[8], ``PRODIGY_STATE``), ``p0`` (bf16, the weight at a parameter's first update) for segments whose ``seg_step`` is
    1, and one fp64 (numerator, denominator) pair per 2048-element chunk in ``partials`` (fp64[2 * chunks])."""
    _need_prodigy_layout("prodigy_moments", p, lo, m, v, seg_start, seg_active, state,
                         (("g", g), ("p0", p0), ("s", s), ("seg_step", seg_step), ("partials", partials)))
    _need(g, BF16, "g"), _need(p0, BF16, "p0"), _need(s, torch.float32, "s"), _need(seg_step, torch.int32, "seg_step")
    _need(partials, torch.float64, "partials")
    if clip_coef is not None:
        _need(clip_coef, torch.float32, "clip_coef")
    n = p.numel()
    if g.numel() < n or p0.numel() != n or s.numel() != n or seg_step.numel() != seg_active.numel() or partials.numel() * 1024 != n:
        raise RuntimeError("orv_amd.ops: prodigy_moments buffers do not share one flat layout (partials: one fp64 pair per 2048 elements)")
    check(lib().orv_prodigy_moments(_p(p), _p(lo), _p(g), _p(p0), _p(m), _p(v), _p(s), n, _p(seg_start), _p(seg_active), _p(seg_step),
                                    seg_active.numel(), _p(state), _p(partials), float(lr), float(beta1), float(beta2), float(beta3),
                                    float(weight_decay), int(bool(decouple)), int(bool(safeguard_warmup)), int(bool(use_bias_correction)),
                                    float(d0), _p(clip_coef), _stream()), "orv_prodigy_moments")


def prodigy_recurrence(state, partials, lr, beta1, beta2, beta3, use_bias_correction=False, d0=1e-6, d_coef=1.0, growth_rate=float("inf")):
    """Launch 2 (``orv_prodigy_recurrence``): adds the pairs of ``partials`` in fp64 and advances ``state`` (d, d_max, d_numerator, d_hat, k),
    or raises its skip flag when the denominator is 0."""
    _need(state, torch.float64, "state"), _need(partials, torch.float64, "partials")
    if (not state.is_contiguous() or not partials.is_contiguous() or state.numel() != len(PRODIGY_STATE) or partials.numel() < 2
            or partials.numel() % 2):
        raise RuntimeError(f"orv_amd.ops: prodigy_recurrence wants contiguous state fp64[{len(PRODIGY_STATE)}] and partials fp64[2 * chunks]")
    check(lib().orv_prodigy_recurrence(_p(state), _p(partials), partials.numel() // 2, float(lr), float(beta1), float(beta2), float(beta3),
                                       int(bool(use_bias_correction)), float(d0), float(d_coef), float(growth_rate), _stream()),
          "orv_prodigy_recurrence")


def prodigy_update(p, lo, m, v, seg_start, seg_active, state, eps, weight_decay=0.0, decouple=True):
    """Launch 3 (``orv_prodigy_update``): the weight update on the split fp32 master (``p`` bf16 + ``lo`` int16, the format of
    ``adamw_flat_ex`` mode 1) with the NEW ``d`` and this step's ``dlr`` from ``state``; nothing when the skip flag is set."""
    _need_prodigy_layout("prodigy_update", p, lo, m, v, seg_start, seg_active, state)
    check(lib().orv_prodigy_update(_p(p), _p(lo), _p(m), _p(v), p.numel(), _p(seg_start), _p(seg_active), seg_active.numel(), _p(state),
                                   float(eps), float(weight_decay), int(bool(decouple)), _stream()), "orv_prodigy_update")


CAME_LAUNCHES = ("q_sums", "statistics", "usq_sums", "k", "m_and_s_sums", "confidence", "weights")     # `which` of orv_came_launch
CAME_TILE = (64, 256)                    # rows x columns of one workgroup's tile of a factored matrix (orv_amd/csrc/optim_came.hip)
CAME_GEOM = ("B", "R", "C", "tile0", "mat0", "row0", "col0", "v0", "rowp0", "colp0", "numel", "pad")


def came_geometry(shapes):
    """The geometry table of ``orv_came_*`` for parameters of these shapes, one flat segment each (host arithmetic only): a shape of two or
    more dimensions is ``B = prod(shape[:-2])`` matrices of ``R x C`` with row / column statistics, anything else is unfactored (``R = 0``)
    and keeps one value of ``v`` per element, padded to 2048.  -> dict: ``table`` (rows of ``CAME_GEOM``), the totals ``n_tiles``,
    ``n_mats``, ``n_rows``, ``n_cols``, ``n_v``, ``n_rowp``, ``n_colp`` and ``n_scratch``, the fp32 values of scratch one step needs."""
    tr, tc = CAME_TILE
    t = dict(n_tiles=0, n_mats=0, n_rows=0, n_cols=0, n_v=0, n_rowp=0, n_colp=0)
    table = []
    for shape in shapes:
        shape = tuple(int(d) for d in shape)
        numel = 1
        for d in shape:
            numel *= d
        if numel <= 0:
            raise ValueError(f"orv_amd.ops.came_geometry: a parameter of shape {shape} has no elements")
        if len(shape) >= 2:
            R, C = shape[-2:]
            B = numel // (R * C)
            nrt, nct = -(-R // tr), -(-C // tc)
            own = dict(n_tiles=B * nrt * nct, n_mats=B, n_rows=B * R, n_cols=B * C, n_v=0, n_rowp=B * R * nct, n_colp=B * C * nrt)
        else:
            B, R, C = 1, 0, 0
            chunks = -(-numel // 2048)
            own = dict(n_tiles=chunks, n_mats=0, n_rows=0, n_cols=0, n_v=chunks * 2048, n_rowp=0, n_colp=0)
        table.append([B, R, C, t["n_tiles"], t["n_mats"], t["n_rows"], t["n_cols"], t["n_v"], t["n_rowp"], t["n_colp"], numel, 0])
        for k, x in own.items():
            t[k] += x
    t["n_scratch"] = t["n_rowp"] + t["n_colp"] + t["n_tiles"] + t["n_rows"] + t["n_cols"] + 2 * len(table)
    t["table"] = table
    return t


def came_step(p, g, m, stats, seg_start, seg_active, geom, sizes, scratch, lr, betas, eps=(1e-30, 1e-16), clip_threshold=1.0,
              weight_decay=0.0, clip_coef=None, lo=None, mode=0, which=None):
    """One fused CAME step (``orv_came_step``: seven stream-ordered launches) on the flat layout of ``adamw_flat_ex``, or
    the single launch ``which`` (an index or a name of ``CAME_LAUNCHES``; ``orv_came_launch``).  ``stats``: dict of the fp32 statistics
    ``r``, ``c``, ``res_r``, ``res_c`` (``sizes["n_rows"]`` / ``["n_cols"]`` values) and ``v`` (``sizes["n_v"]``; an entry of size 0 may be
    None); ``geom``: the int64 device copy of ``came_geometry(...)["table"]``, ``sizes`` that dict; ``scratch``: fp32, at least
    ``sizes["n_scratch"]`` values; ``mode`` 0 (bf16 weights, nearest-even) or 1 (split fp32 master, needs ``lo``)."""
    from ._lib import Came
    mode = ADAMW_MODES.get(mode, mode)
    _need(p, BF16, "p"), _need(g, BF16, "g"), _need(m, torch.float32, "m"), _need(scratch, torch.float32, "scratch")
    _need(seg_start, torch.int64, "seg_start"), _need(seg_active, torch.uint8, "seg_active"), _need(geom, torch.int64, "geom")
    named = [("p", p), ("g", g), ("m", m), ("scratch", scratch), ("seg_start", seg_start), ("seg_active", seg_active), ("geom", geom)]
    if lo is not None:
        named.append(("lo", _need(lo, torch.int16, "lo")))
    if clip_coef is not None:
        named.append(("clip_coef", _need(clip_coef, torch.float32, "clip_coef")))
    want = {"r": sizes["n_rows"], "c": sizes["n_cols"], "res_r": sizes["n_rows"], "res_c": sizes["n_cols"], "v": sizes["n_v"]}
    for k, cnt in want.items():
        s = stats.get(k)
        if s is None and cnt == 0:
            continue
        if s is None or _need(s, torch.float32, k).numel() != cnt:
            raise RuntimeError(f"orv_amd.ops: came_step statistic `{k}` must hold {cnt} fp32 values")
        named.append((k, s))
    for name, t in named:
        if not t.is_contiguous():
            raise RuntimeError(f"orv_amd.ops: `{name}` must be contiguous")
    nseg, n = seg_active.numel(), p.numel()
    if (g.numel() < n or m.numel() != n or seg_start.numel() != nseg + 1 or geom.numel() != nseg * len(CAME_GEOM)
            or len(sizes["table"]) != nseg or (lo is not None and lo.numel() != n)):
        raise RuntimeError("orv_amd.ops: came_step buffers do not share one flat layout")
    d = Came(p=_p(p), lo=_p(lo), g=_p(g), m=_p(m), r=_p(stats.get("r")), c=_p(stats.get("c")), res_r=_p(stats.get("res_r")),
             res_c=_p(stats.get("res_c")), v=_p(stats.get("v")), n=n, n_rows=sizes["n_rows"], n_cols=sizes["n_cols"], n_v=sizes["n_v"],
             seg_start=_p(seg_start), seg_active=_p(seg_active), nseg=nseg, geom=_p(geom), n_tiles=sizes["n_tiles"], n_mats=sizes["n_mats"],
             n_rowp=sizes["n_rowp"], n_colp=sizes["n_colp"], scratch=_p(scratch), n_scratch=scratch.numel(), clip_coef=_p(clip_coef),
             lr=float(lr), beta1=float(betas[0]), beta2=float(betas[1]), beta3=float(betas[2]), eps1=float(eps[0]), eps2=float(eps[1]),
             clip_threshold=float(clip_threshold), weight_decay=float(weight_decay), mode=int(mode))
    if which is None:
        check(lib().orv_came_step(d, _stream()), "orv_came_step")
    else:
        which = CAME_LAUNCHES.index(which) if isinstance(which, str) else int(which)
        check(lib().orv_came_launch(d, which, _stream()), "orv_came_launch")


def _need_ema_layout(what, named):
    """Every buffer of an EMA launch: on the GPU, of its dtype, contiguous, 16-byte aligned, all of one length that is a multiple of 2048."""
    n = named[0][1].numel()
    for name, t, dtype in named:
        if t is None:
            continue
        _need(t, dtype, name)
        if not t.is_contiguous():
            raise RuntimeError(f"orv_amd.ops: `{name}` must be contiguous")
        if t.numel() != n:
            raise RuntimeError(f"orv_amd.ops: {what}: `{name}` holds {t.numel()} elements, `{named[0][0]}` {n} (one flat layout)")
        if t.data_ptr() % 16:
            raise RuntimeError(f"orv_amd.ops: {what}: `{name}` must be 16-byte aligned (the kernel moves 16 bytes per access)")
    if n == 0 or n % 2048:
        raise RuntimeError(f"orv_amd.ops: {what}: {n} elements; the flat layout is a positive multiple of 2048 (pad every segment)")
    return n


def ema_update(shadow, p, lo=None, one_minus_decay=0.0):
    """``shadow <- shadow - one_minus_decay * (shadow - theta)`` over a whole flat buffer in one launch (``orv_ema_update``): ``shadow``
    fp32 in the layout of ``p`` (bf16), ``theta`` the fp32 master ``p | lo`` where ``lo`` (int16) is given, else ``fp32(p)``."""
    n = _need_ema_layout("ema_update", (("shadow", shadow, torch.float32), ("p", p, BF16), ("lo", lo, torch.int16)))
    omd = float(one_minus_decay)
    if not 0.0 <= omd <= 1.0:
        raise RuntimeError(f"orv_amd.ops: ema_update: one_minus_decay={one_minus_decay} must lie in [0, 1]")
    check(lib().orv_ema_update(_p(shadow), _p(p), _p(lo), n, omd, _stream()), "orv_ema_update")


def ema_swap_in(p, shadow, lo=None, stash_p=None, stash_lo=None, zero_lo=False):
    """``stash_p <- p``, ``stash_lo <- lo`` (where given), then ``p <- bf16_rne(shadow)`` and, with ``zero_lo``, ``lo <- 0`` - one launch
    (``orv_ema_swap_in``)."""
    n = _need_ema_layout("ema_swap_in", (("p", p, BF16), ("shadow", shadow, torch.float32), ("lo", lo, torch.int16),
                                         ("stash_p", stash_p, BF16), ("stash_lo", stash_lo, torch.int16)))
    if lo is None and (stash_lo is not None or zero_lo):
        raise RuntimeError("orv_amd.ops: ema_swap_in: `stash_lo` / `zero_lo` given without the low-half buffer `lo`")
    if stash_lo is not None and stash_p is None:
        raise RuntimeError("orv_amd.ops: ema_swap_in: `stash_lo` given without `stash_p`")
    check(lib().orv_ema_swap_in(_p(p), _p(lo), _p(shadow), _p(stash_p), _p(stash_lo), n, int(bool(zero_lo)), _stream()), "orv_ema_swap_in")


STATE8_FORMATS = {"m": 0, "v": 1}         # first moment: e4m3fn, second moment: e5m2 (orv_amd/csrc/optim_s8.hip)


def _need_state8(q, exps, what):
    _need(q, torch.uint8, what), _need(exps, torch.uint8, what + "_exp")
    if not q.is_contiguous() or not exps.is_contiguous():
        raise RuntimeError(f"orv_amd.ops: `{what}` and `{what}_exp` must be contiguous")
    if q.numel() % 256 or exps.numel() * 256 != q.numel():
        raise RuntimeError(f"orv_amd.ops: `{what}` holds {q.numel()} elements, `{what}_exp` {exps.numel()} scale bytes (one per 256)")


def adamw_flat_s8(p, g, m8, v8, m_exp, v_exp, seg_start, seg_active, lr, beta1, beta2, eps, weight_decay, step, clip_coef=None,
                  seg_step=None, lo=None, mode=0, seed=0):
    """``adamw_flat_ex`` on block-scaled fp8 moments: ``m8`` / ``v8`` uint8 in the layout of ``p`` (e4m3fn / e5m2 bytes), ``m_exp`` /
    ``v_exp`` one scale byte per 256 elements.  ``mode`` as ``ADAMW_MODES`` (0 here: nearest-even bf16 of the fp32 result)."""
    mode = ADAMW_MODES.get(mode, mode)
    _need(p, BF16, "p"), _need(g, BF16, "g"), _need_state8(m8, m_exp, "m8"), _need_state8(v8, v_exp, "v8")
    _need(seg_start, torch.int64, "seg_start"), _need(seg_active, torch.uint8, "seg_active")
    if seg_step is not None:
        _need(seg_step, torch.int32, "seg_step")
    if clip_coef is not None:
        _need(clip_coef, torch.float32, "clip_coef")
    if lo is not None:
        _need(lo, torch.int16, "lo")
        if lo.numel() != p.numel():
            raise RuntimeError(f"orv_amd.ops: `lo` holds {lo.numel()} elements, `p` {p.numel()}")
    for name, t in (("p", p), ("g", g), ("seg_start", seg_start), ("seg_active", seg_active), ("seg_step", seg_step), ("lo", lo)):
        if t is not None and not t.is_contiguous():
            raise RuntimeError(f"orv_amd.ops: `{name}` must be contiguous")
    if g.numel() < p.numel() or m8.numel() != p.numel() or v8.numel() != p.numel() or seg_start.numel() != seg_active.numel() + 1:
        raise RuntimeError("orv_amd.ops: adamw_flat_s8 buffers do not share one flat layout")
    check(lib().orv_adamw_flat_s8(_p(p), _p(g), _p(m8), _p(v8), _p(m_exp), _p(v_exp), p.numel(), _p(seg_start), _p(seg_active),
                                  _p(seg_step), seg_active.numel(), float(lr), float(beta1), float(beta2), float(eps),
                                  float(weight_decay), int(step), _p(clip_coef), _p(lo), int(mode), int(seed) & 0xFFFFFFFF, _stream()),
          "orv_adamw_flat_s8")


ADAMW_MAX_GROUPS = _ADAMW_MAX_GROUPS
GUARD_REPORT = ("ss",) + tuple(f"group{j}" for j in range(ADAMW_MAX_GROUPS)) + ("skip_count", "skipped")      # the fp64[11] of orv_step_guard


def _adamw_groups(seg_group, seg_active, lrs, weight_decays, max_group=None):
    """The by-value table of ``orv_adamw_flat_groups`` from two equally long sequences; ``max_group`` is the largest value in ``seg_group``
    as the caller knows it from building that table on the host (``None``: read it from the device, one host sync - tests and tools)."""
    lrs, weight_decays = [float(x) for x in lrs], [float(x) for x in weight_decays]
    if not 1 <= len(lrs) <= ADAMW_MAX_GROUPS or len(weight_decays) != len(lrs):
        raise RuntimeError(f"orv_amd.ops: {len(lrs)} learning rates and {len(weight_decays)} weight decays (supported: 1..{ADAMW_MAX_GROUPS} "
                           "groups, one of each per group)")
    _need(seg_group, torch.uint8, "seg_group")
    if not seg_group.is_contiguous() or seg_group.numel() != seg_active.numel():
        raise RuntimeError(f"orv_amd.ops: `seg_group` must be contiguous and hold one byte per segment ({seg_active.numel()})")
    if max_group is None:
        max_group = int(seg_group.max().item())
    if max_group >= len(lrs):
        raise RuntimeError(f"orv_amd.ops: `seg_group` names group {max_group}, the table holds {len(lrs)} (every value must be < ngroups)")
    tab = AdamwGroups()
    tab.ngroups = len(lrs)
    for j, (a, b) in enumerate(zip(lrs, weight_decays)):
        tab.lr[j], tab.weight_decay[j] = a, b
    return tab


def adamw_flat_groups(p, g, m, v, seg_start, seg_active, seg_group, lrs, weight_decays, beta1, beta2, eps, step, clip_coef=None,
                      seg_step=None, lo=None, mode=0, seed=0, max_group=None):
    """``adamw_flat_ex`` with one ``(lr, weight_decay)`` per parameter group: ``seg_group`` uint8 on the device names the group of every
    segment, ``lrs`` / ``weight_decays`` are host sequences (1..8 entries) that travel by value with the launch."""
    mode = ADAMW_MODES.get(mode, mode)
    _need(p, BF16, "p"), _need(g, BF16, "g"), _need(m, torch.float32, "m"), _need(v, torch.float32, "v")
    _need(seg_start, torch.int64, "seg_start"), _need(seg_active, torch.uint8, "seg_active")
    if seg_step is not None:
        _need(seg_step, torch.int32, "seg_step")
    if clip_coef is not None:
        _need(clip_coef, torch.float32, "clip_coef")
    if lo is not None:
        _need(lo, torch.int16, "lo")
        if lo.numel() != p.numel():
            raise RuntimeError(f"orv_amd.ops: `lo` holds {lo.numel()} elements, `p` {p.numel()}")
    for name, t in (("p", p), ("g", g), ("m", m), ("v", v), ("seg_start", seg_start), ("seg_active", seg_active), ("seg_step", seg_step),
                    ("lo", lo)):
        if t is not None and not t.is_contiguous():
            raise RuntimeError(f"orv_amd.ops: `{name}` must be contiguous")
    if g.numel() < p.numel() or m.numel() != p.numel() or v.numel() != p.numel() or seg_start.numel() != seg_active.numel() + 1:
        raise RuntimeError("orv_amd.ops: adamw_flat_groups buffers do not share one flat layout")
    tab = _adamw_groups(seg_group, seg_active, lrs, weight_decays, max_group)
    check(lib().orv_adamw_flat_groups(_p(p), _p(g), _p(m), _p(v), p.numel(), _p(seg_start), _p(seg_active), _p(seg_step),
                                      seg_active.numel(), _p(seg_group), tab, float(beta1), float(beta2), float(eps), int(step),
                                      _p(clip_coef), _p(lo), int(mode), int(seed) & 0xFFFFFFFF, _stream()), "orv_adamw_flat_groups")


def adamw_flat_s8_groups(p, g, m8, v8, m_exp, v_exp, seg_start, seg_active, seg_group, lrs, weight_decays, beta1, beta2, eps, step,
                         clip_coef=None, seg_step=None, lo=None, mode=0, seed=0, max_group=None, common_count=0):
    """``adamw_flat_s8`` with one ``(lr, weight_decay)`` per parameter group (see ``adamw_flat_groups``).  ``common_count``: the
    per-segment count most segments are at when it is not ``step`` (after a skipped step); it only spares the kernel its own bias
    corrections, the result does not depend on it."""
    mode = ADAMW_MODES.get(mode, mode)
    _need(p, BF16, "p"), _need(g, BF16, "g"), _need_state8(m8, m_exp, "m8"), _need_state8(v8, v_exp, "v8")
    _need(seg_start, torch.int64, "seg_start"), _need(seg_active, torch.uint8, "seg_active")
    if seg_step is not None:
        _need(seg_step, torch.int32, "seg_step")
    if clip_coef is not None:
        _need(clip_coef, torch.float32, "clip_coef")
    if lo is not None:
        _need(lo, torch.int16, "lo")
        if lo.numel() != p.numel():
            raise RuntimeError(f"orv_amd.ops: `lo` holds {lo.numel()} elements, `p` {p.numel()}")
    for name, t in (("p", p), ("g", g), ("seg_start", seg_start), ("seg_active", seg_active), ("seg_step", seg_step), ("lo", lo)):
        if t is not None and not t.is_contiguous():
            raise RuntimeError(f"orv_amd.ops: `{name}` must be contiguous")
    if g.numel() < p.numel() or m8.numel() != p.numel() or v8.numel() != p.numel() or seg_start.numel() != seg_active.numel() + 1:
        raise RuntimeError("orv_amd.ops: adamw_flat_s8_groups buffers do not share one flat layout")
    tab = _adamw_groups(seg_group, seg_active, lrs, weight_decays, max_group)
    check(lib().orv_adamw_flat_s8_groups(_p(p), _p(g), _p(m8), _p(v8), _p(m_exp), _p(v_exp), p.numel(), _p(seg_start), _p(seg_active),
                                         _p(seg_step), seg_active.numel(), _p(seg_group), tab, float(beta1), float(beta2), float(eps),
                                         int(step), int(common_count), _p(clip_coef), _p(lo), int(mode), int(seed) & 0xFFFFFFFF,
                                         _stream()), "orv_adamw_flat_s8_groups")


def segment_sumsq(g, seg_start, out):
    """``out[i]`` (fp64) = the sum of squares of the bf16 elements ``g[seg_start[i]:seg_start[i + 1]]``, one launch, in the fixed order
    stated in ``orv_amd/csrc/optim_groups.hip``.  The caller guarantees that ``seg_start`` is ascending and ends inside ``g``."""
    _need(g, BF16, "g"), _need(seg_start, torch.int64, "seg_start"), _need(out, torch.float64, "out")
    if not (g.is_contiguous() and seg_start.is_contiguous() and out.is_contiguous()) or seg_start.numel() != out.numel() + 1:
        raise RuntimeError(f"orv_amd.ops: segment_sumsq wants contiguous buffers and len(seg_start) == len(out) + 1 "
                           f"(got {seg_start.numel()} and {out.numel()})")
    check(lib().orv_segment_sumsq(_p(g), _p(seg_start), out.numel(), _p(out), _stream()), "orv_segment_sumsq")


def step_guard(seg_ss, seg_group, seg_active, clip_coef, report, max_grad_norm, inv_world=1.0, skip_nonfinite=False):
    """The device-side decisions of one optimizer step (``orv_step_guard``): global and per-group sums of ``seg_ss`` in index order, the
    clip coefficient, and - with ``skip_nonfinite`` and a non-finite sum - a cleared ``seg_active`` and a counted skip.  ``report``: fp64
    ``[len(GUARD_REPORT)]``, zeroed once by the caller."""
    _need(seg_ss, torch.float64, "seg_ss"), _need(seg_group, torch.uint8, "seg_group"), _need(seg_active, torch.uint8, "seg_active")
    _need(clip_coef, torch.float32, "clip_coef"), _need(report, torch.float64, "report")
    n = seg_ss.numel()
    if seg_group.numel() != n or seg_active.numel() != n or report.numel() != len(GUARD_REPORT) or clip_coef.numel() < 1:
        raise RuntimeError(f"orv_amd.ops: step_guard wants {n} bytes in seg_group and seg_active, {len(GUARD_REPORT)} doubles in report")
    for name, t in (("seg_ss", seg_ss), ("seg_group", seg_group), ("seg_active", seg_active), ("report", report)):
        if not t.is_contiguous():
            raise RuntimeError(f"orv_amd.ops: `{name}` must be contiguous")
    check(lib().orv_step_guard(_p(seg_ss), _p(seg_group), n, float(max_grad_norm), float(inv_world), int(bool(skip_nonfinite)),
                               _p(seg_active), _p(clip_coef), _p(report), _stream()), "orv_step_guard")


def state8_quantize(x, q, exps, fmt, seed=0, step=0):
    """fp32 ``x`` -> the bytes ``adamw_flat_s8`` stores for these moment values at (``seed``, ``step``, flat index); ``fmt`` "m" / 0
    (e4m3fn) or "v" / 1 (e5m2).  ``x.numel()`` must be a multiple of 256."""
    _need(x, torch.float32, "x"), _need_state8(q, exps, "q")
    if not x.is_contiguous() or x.numel() != q.numel():
        raise RuntimeError(f"orv_amd.ops: `x` must be contiguous and hold the {q.numel()} elements of `q`")
    check(lib().orv_state8_quantize(_p(x), _p(q), _p(exps), x.numel(), int(STATE8_FORMATS.get(fmt, fmt)), int(seed) & 0xFFFFFFFF,
                                    int(step), _stream()), "orv_state8_quantize")


def state8_dequantize(q, exps, x, fmt):
    """The fp32 values of block-scaled fp8 moments (exact)."""
    _need(x, torch.float32, "x"), _need_state8(q, exps, "q")
    if not x.is_contiguous() or x.numel() != q.numel():
        raise RuntimeError(f"orv_amd.ops: `x` must be contiguous and hold the {q.numel()} elements of `q`")
    check(lib().orv_state8_dequantize(_p(q), _p(exps), _p(x), x.numel(), int(STATE8_FORMATS.get(fmt, fmt)), _stream()),
          "orv_state8_dequantize")


def sumsq(g, out):
    check(lib().orv_sumsq(_p(g), g.numel(), _p(out), _stream()), "orv_sumsq")


def head_transpose(src, col0, dst, B, S, H, s_pad, ld=None):
    check(lib().orv_head_transpose(_p(src), ld or src.shape[-1], col0, _p(dst), B, S, H, s_pad, _stream()),
          "orv_head_transpose")
    return dst


def attention_bwd(qkv, qT, kT, out, dout, doT, lse, neg_lse2, neg_delta, dqkv, B, S, H, s_pad, scale):
    check(lib().orv_attention_bwd(_p(qkv), 3 * H * 64, _p(qT), _p(kT), _p(out), _p(dout), H * 64, _p(doT), _p(lse),
                                  _p(neg_lse2), _p(neg_delta), _p(dqkv), 3 * H * 64, B, S, H, s_pad, float(scale), _stream()),
          "orv_attention_bwd")
    return dqkv


def qkv_prep_bwd(qkv_raw, dqkv, gq, gk, rope, dgq, dbq, dgk, dbk, B, S, H, n_text, eps):
    cos = sin = None
    if rope is not None:
        cos, sin = rope
    nblk = ((S + 63) // 64) * H * B
    scratch = torch.empty(nblk * 256, dtype=torch.float32, device=dqkv.device)
    check(lib().orv_qkv_prep_bwd(_p(qkv_raw), _p(dqkv), _p(gq), _p(gk), _p(cos), _p(sin), _p(dgq), _p(dbq), _p(dgk), _p(dbk),
                                 _p(scratch), B, S, H, n_text, float(eps), _stream()), "orv_qkv_prep_bwd")


# ---- VAE building blocks (vae.hip): channels-last activations [B, T, H, W, C] ----
def vae_im2col(src, dst, B, Ts, Hs, Ws, C, T, H, W, kt, kh, kw, stride, pad_lo, ups_s, ups_t, t_shift, Kpad, m0, mc):
    _need(src, BF16, "src"), _need(dst, BF16, "dst")
    check(lib().orv_vae_im2col(_p(src), _p(dst), B, Ts, Hs, Ws, C, T, H, W, kt, kh, kw, stride, pad_lo, int(ups_s), int(ups_t),
                               int(t_shift), Kpad, int(m0), int(mc), _stream()), "orv_vae_im2col")
    return dst


def conv_gemm(src, Wp, bias, out, B, Ts, Hs, Ws, C, T, H, W, kt, kh, kw, stride, pad_lo, ups_s, ups_t, t_shift, N, R=None, ldr=None):
    """Implicit-GEMM convolution (no patch matrix): out[B*T*H*W, N] = conv(src) + bias (+ R)."""
    from ._lib import Conv
    _need(src, BF16, "src"), _need(Wp, BF16, "W"), _need(out, BF16, "out")
    M, K = B * T * H * W, kt * kh * kw * C
    g = Gemm()
    g.A, g.lda, g.W, g.ldw, g.bias = None, 0, _p(Wp), K, _p(bias)
    g.C, g.ldc, g.M, g.N, g.K, g.epilogue = _p(out), N, M, N, K, 2 if R is not None else 0
    g.R, g.ldr, g.r_mod, g.gate = _p(R), ldr or N, 0, None
    g.grp, g.cmap = Groups(0, 0, 0), RowMap(0, 0, 0)
    c = Conv(_p(src), B, Ts, Hs, Ws, C, T, H, W, kt, kh, kw, stride, pad_lo, int(ups_s), int(ups_t), int(t_shift))
    check(lib().orv_conv_gemm_bf16(g, c, _stream()), "orv_conv_gemm_bf16")
    return out


def vae_groupnorm_stats(x, B, N, C, G):
    """-> sums fp32 [B, G, 2] (sum, sum of squares per group), deterministic."""
    _need(x, BF16, "x")
    sums = torch.empty(B, G, 2, dtype=torch.float32, device=x.device)
    scratch = torch.empty(lib().orv_vae_groupnorm_scratch(B, int(N), C, G), dtype=torch.float32, device=x.device)
    check(lib().orv_vae_groupnorm_stats(_p(x), _p(sums), _p(scratch), B, int(N), C, G, _stream()), "orv_vae_groupnorm_stats")
    return sums


def vae_blend(a, b, extent, horizontal):
    """In-place seam blend of channels-last tiles a, b [B, T, H, W, C] (diffusers blend_v / blend_h): see orv_vae_blend."""
    _need(a, BF16, "a"), _need(b, BF16, "b")
    if not (a.is_contiguous() and b.is_contiguous()):
        raise ValueError("vae_blend: tiles must be contiguous")
    B, T, Ha, Wa, C = a.shape
    _, _, Hb, Wb, _ = b.shape
    check(lib().orv_vae_blend(_p(a), _p(b), B * T, Ha, Wa, Hb, Wb, C, int(extent), int(bool(horizontal)), _stream()), "orv_vae_blend")
    return b


def vae_norm_apply(x, out, sums, gamma, beta, zy, zb, B, T, H, W, C, G, Tz, hz, wz, eps, silu, out_lead=0):
    """``out`` is [B, out_lead + T, H, W, C]; frames [0, out_lead) of each clip are left untouched."""
    _need(x, BF16, "x"), _need(out, BF16, "out"), _need(gamma, BF16, "gamma"), _need(beta, BF16, "beta")
    check(lib().orv_vae_norm_apply(_p(x), _p(out), _p(sums), _p(gamma), _p(beta), _p(zy), _p(zb), B, T, H, W, C, G, Tz, hz, wz,
                                   float(eps), int(bool(silu)), int(out_lead), _stream()), "orv_vae_norm_apply")
    return out


# ---- T5 text encoder (t5.hip) ----
def t5_attention_max_seq() -> int:
    """Longest sequence ``t5_attention_fwd`` takes."""
    return int(lib().orv_t5_attention_max_seq())


def t5_attention_fwd(qkv, bias_rel, out, B, S, H, ld_qkv=None, ld_out=None):
    """T5 self-attention: ``out = softmax(q k^T + bias) v`` with no score scale; ``qkv`` bf16 [B S, 3 H 64] packed as ``attention_fwd`` reads it,
    ``bias_rel`` fp32 [H, 2S - 1] (entry j - i + S - 1: query i, key j), ``out`` bf16 [B S, H 64]."""
    _need(qkv, BF16, "qkv"), _need(out, BF16, "out"), _need(bias_rel, torch.float32, "bias_rel")
    if not bias_rel.is_contiguous() or bias_rel.numel() != H * (2 * S - 1):
        raise ValueError(f"t5_attention_fwd: bias_rel must be contiguous [H, 2S - 1] = [{H}, {2 * S - 1}] (got {tuple(bias_rel.shape)})")
    with _timed(("t5_attention", B, S, H)):
        check(lib().orv_t5_attention_fwd(_p(qkv), ld_qkv or 3 * H * 64, _p(bias_rel), _p(out), ld_out or H * 64, B, S, H, _stream()),
              "orv_t5_attention_fwd")
    return out


def t5_rmsnorm(x, w, y, M, D, eps, ldx=None, ldy=None):
    """``y = w * bf16(x * rsqrt(mean(x^2) + eps))`` over rows of bf16 [M, D] (T5LayerNorm: no mean subtraction, no bias)."""
    _need(x, BF16, "x"), _need(w, BF16, "w"), _need(y, BF16, "y")
    if w.numel() != D or not w.is_contiguous():
        raise ValueError(f"t5_rmsnorm: w must hold {D} contiguous elements")
    check(lib().orv_t5_rmsnorm(_p(x), ldx or D, _p(w), _p(y), ldy or D, M, D, float(eps), _stream()), "orv_t5_rmsnorm")
    return y


def geglu(h, out, M, F, ldh=None, ldo=None):
    """``out[:, f] = gelu_tanh(h[:, f]) * h[:, F + f]`` (bf16 [M, 2F] -> bf16 [M, F], fp32 inside, one rounding)."""
    _need(h, BF16, "h"), _need(out, BF16, "out")
    check(lib().orv_geglu(_p(h), ldh or 2 * F, _p(out), ldo or F, M, F, _stream()), "orv_geglu")
    return out


# ---- Gaussian rasterizer (gs_render.hip) ----
def _need_c(t, dtype, name):
    if not t.is_contiguous():
        raise ValueError(f"orv_amd.ops: `{name}` must be contiguous")
    return _need(t, dtype, name)


def _same_device(*named):
    dev = named[0][0].device
    for t, n in named:
        if t.device != dev:
            raise RuntimeError(f"orv_amd.ops: `{n}` is on {t.device} but `{named[0][1]}` is on {dev}; all operands of one call share a device")


def gs_preprocess(means3D, scales, rotations, opacities, viewmatrix, projmatrix, H, W, tanfovx, tanfovy, scale_modifier):
    """Project N Gaussians: -> (xy [N,2], conic_opacity [N,4], depth [N], radii [N] int32, rect [N,4] int32, tiles_touched [N] int32)."""
    f32 = torch.float32
    for t, n in ((means3D, "means3D"), (scales, "scales"), (rotations, "rotations"), (opacities, "opacities"), (viewmatrix, "viewmatrix"),
                 (projmatrix, "projmatrix")):
        _need_c(t, f32, n)
    _same_device((means3D, "means3D"), (scales, "scales"), (rotations, "rotations"), (opacities, "opacities"), (viewmatrix, "viewmatrix"),
                 (projmatrix, "projmatrix"))
    if means3D.dim() != 2 or means3D.shape[1] != 3:
        raise ValueError(f"gs_preprocess: means3D must be [N,3] (got {tuple(means3D.shape)})")
    N, dev = means3D.shape[0], means3D.device
    if scales.numel() != 3 * N or rotations.numel() != 4 * N or opacities.numel() != N or viewmatrix.numel() != 16 or projmatrix.numel() != 16:
        raise ValueError("gs_preprocess: means3D [N,3], scales [N,3], rotations [N,4], opacities [N,1], viewmatrix / projmatrix [4,4]")
    xy, conic_op, depth = torch.empty(N, 2, dtype=f32, device=dev), torch.empty(N, 4, dtype=f32, device=dev), torch.empty(N, dtype=f32, device=dev)
    radii, rect = torch.empty(N, dtype=torch.int32, device=dev), torch.empty(N, 4, dtype=torch.int32, device=dev)
    tiles = torch.empty(N, dtype=torch.int32, device=dev)
    check(lib().orv_gs_preprocess(_p(means3D), _p(scales), _p(rotations), _p(opacities), _p(viewmatrix), _p(projmatrix), N, int(H), int(W),
                                  float(tanfovx), float(tanfovy), float(scale_modifier), _p(xy), _p(conic_op), _p(depth), _p(radii), _p(rect),
                                  _p(tiles), _stream()), "orv_gs_preprocess")
    return xy, conic_op, depth, radii, rect, tiles


def gs_tile_keys(rect, depth, offsets, H, W, L):
    """-> (keys int64 [L], gaussian_idx int32 [L]); ``offsets`` = inclusive int64 prefix sum of tiles_touched, ``L`` its last entry."""
    _need_c(rect, torch.int32, "rect"), _need_c(depth, torch.float32, "depth"), _need_c(offsets, torch.int64, "offsets")
    _same_device((rect, "rect"), (depth, "depth"), (offsets, "offsets"))
    if rect.dim() != 2 or rect.shape[1] != 4 or depth.numel() != rect.shape[0] or offsets.numel() != rect.shape[0]:
        raise ValueError("gs_tile_keys: rect [N,4], depth [N], offsets [N]")
    keys = torch.empty(L, dtype=torch.int64, device=rect.device)
    idx = torch.empty(L, dtype=torch.int32, device=rect.device)
    check(lib().orv_gs_tile_keys(_p(rect), _p(depth), _p(offsets), rect.shape[0], int(H), int(W), int(L), _p(keys), _p(idx), _stream()),
          "orv_gs_tile_keys")
    return keys, idx


def gs_tile_ranges(sorted_keys, H, W):
    """-> ranges int32 [tiles, 2]: [start, end) of each 16x16 tile's run in ``sorted_keys``; (0, 0) for a tile nothing covers."""
    _need_c(sorted_keys, torch.int64, "sorted_keys")
    ranges = torch.zeros(((H + 15) // 16) * ((W + 15) // 16), 2, dtype=torch.int32, device=sorted_keys.device)
    check(lib().orv_gs_tile_ranges(_p(sorted_keys), sorted_keys.numel(), int(H), int(W), _p(ranges), _stream()), "orv_gs_tile_ranges")
    return ranges


def gs_render(ranges, point_list, xy, conic_opacity, depth, colors, features, bg, H, W):
    """Blend every tile's list: -> (color [3,H,W], feature [F,H,W], depth [1,H,W], alpha [1,H,W]); ``features`` None or [N,0] = no feature plane."""
    f32 = torch.float32
    _need_c(ranges, torch.int32, "ranges"), _need_c(point_list, torch.int32, "point_list"), _need_c(bg, f32, "bg")
    for t, n in ((xy, "xy"), (conic_opacity, "conic_opacity"), (depth, "depth"), (colors, "colors")):
        _need_c(t, f32, n)
    N = xy.shape[0]
    F = 0 if features is None else int(features.shape[1])
    if F:
        _need_c(features, f32, "features")
    _same_device((ranges, "ranges"), (point_list, "point_list"), (bg, "bg"), (xy, "xy"), (conic_opacity, "conic_opacity"), (depth, "depth"),
                 (colors, "colors"), *(((features, "features"),) if F else ()))
    if xy.numel() != 2 * N or conic_opacity.numel() != 4 * N or depth.numel() != N or ranges.numel() != 2 * ((H + 15) // 16) * ((W + 15) // 16):
        raise ValueError("gs_render: xy [N,2], conic_opacity [N,4], depth [N], ranges [tiles,2]")
    if colors.numel() != 3 * N or (F and features.shape[0] != N) or bg.numel() != 3:
        raise ValueError("gs_render: colors [N,3], features [N,F], bg [3]")
    dev = ranges.device
    color, feat = torch.empty(3, H, W, dtype=f32, device=dev), torch.empty(F, H, W, dtype=f32, device=dev)
    dep, alpha = torch.empty(1, H, W, dtype=f32, device=dev), torch.empty(1, H, W, dtype=f32, device=dev)
    with _timed(("gs_render", N, F, H, W)):
        check(lib().orv_gs_render(_p(ranges), _p(point_list), point_list.numel(), _p(xy), _p(conic_opacity), _p(depth), _p(colors),
                                  _p(features) if F else None, N, F, _p(bg), int(H), int(W), _p(color), _p(feat) if F else None, _p(dep),
                                  _p(alpha), _stream()), "orv_gs_render")
    return color, feat, dep, alpha


# ---- point-cloud voxelization (voxelize.hip) ----
def voxel_grid_size(voxel_size, coors_range):
    """Cells per axis (x, y, z) of ``coors_range`` [6] cut into ``voxel_size`` [3] (fp32 values): round((hi - lo) / vs) in fp32.  Host only."""
    grid = (ctypes.c_int * 3)()
    check(lib().orv_voxel_grid_size(*[float(v) for v in voxel_size], *[float(v) for v in coors_range], ctypes.addressof(grid)),
          "orv_voxel_grid_size")
    return tuple(grid)


def voxel_coors(points, voxel_size, coors_range, want_keys=True):
    """-> (coors int32 [N,3] in (z, y, x) order, -1 rows for points outside the grid; keys int64 [N] or None)."""
    _need_c(points, torch.float32, "points")
    if points.dim() != 2:
        raise ValueError(f"voxel_coors: points must be [N,C] (got {tuple(points.shape)})")
    N, C = points.shape
    coors = torch.empty(N, 3, dtype=torch.int32, device=points.device)
    keys = torch.empty(N, dtype=torch.int64, device=points.device) if want_keys else None
    check(lib().orv_voxel_coors(_p(points), N, C, *[float(v) for v in voxel_size], *[float(v) for v in coors_range], _p(coors), _p(keys),
                                _stream()), "orv_voxel_coors")
    return coors, keys


def voxel_segments(sorted_keys, order):
    """-> (start int32 [N], seglen int32 [N], first int32 [N]) of the stably sorted keys; ``order`` = the sort's int64 indices."""
    _need_c(sorted_keys, torch.int64, "sorted_keys"), _need_c(order, torch.int64, "order")
    _same_device((sorted_keys, "sorted_keys"), (order, "order"))
    N = sorted_keys.numel()
    if order.numel() != N:
        raise ValueError("voxel_segments: sorted_keys [N], order [N]")
    start, seglen = torch.empty(N, dtype=torch.int32, device=order.device), torch.empty(N, dtype=torch.int32, device=order.device)
    first = torch.zeros(N, dtype=torch.int32, device=order.device)
    check(lib().orv_voxel_segments(_p(sorted_keys), _p(order), N, _p(start), _p(seglen), _p(first), _stream()), "orv_voxel_segments")
    return start, seglen, first


def _voxel_inputs(points, point_coors, order, start, seglen, csum, who):
    _need_c(points, torch.float32, "points"), _need_c(point_coors, torch.int32, "point_coors"), _need_c(order, torch.int64, "order")
    _need_c(start, torch.int32, "start"), _need_c(seglen, torch.int32, "seglen"), _need_c(csum, torch.int32, "csum")
    _same_device((points, "points"), (point_coors, "point_coors"), (order, "order"), (start, "start"), (seglen, "seglen"), (csum, "csum"))
    N = points.shape[0]
    if points.dim() != 2 or point_coors.numel() != 3 * N or any(t.numel() != N for t in (order, start, seglen, csum)):
        raise ValueError(f"{who}: points [N,C], point_coors [N,3], order / start / seglen / csum [N]")
    return N, points.shape[1]


def voxel_scatter(points, point_coors, order, start, seglen, csum, max_points, M):
    """-> (voxels [M, max_points, C] zero-padded, coors int32 [M,3], num_points_per_voxel int32 [M])."""
    N, C = _voxel_inputs(points, point_coors, order, start, seglen, csum, "voxel_scatter")
    dev = points.device
    voxels = torch.zeros(M, max_points, C, dtype=torch.float32, device=dev)
    coors, num = torch.zeros(M, 3, dtype=torch.int32, device=dev), torch.zeros(M, dtype=torch.int32, device=dev)
    with _timed(("voxel_scatter", N, C, max_points, M)):
        check(lib().orv_voxel_scatter(_p(points), _p(point_coors), _p(order), _p(start), _p(seglen), _p(csum), N, C, int(max_points), int(M),
                                      _p(voxels), _p(coors), _p(num), _stream()), "orv_voxel_scatter")
    return voxels, coors, num


def voxel_vote(points, point_coors, order, start, seglen, csum, max_points, M):
    """-> int32 [M,4] = (x, y, z, label) per kept voxel; the last feature of ``points`` holds label + 1."""
    N, C = _voxel_inputs(points, point_coors, order, start, seglen, csum, "voxel_vote")
    head_of = torch.full((M,), -1, dtype=torch.int32, device=points.device)
    out = torch.empty(M, 4, dtype=torch.int32, device=points.device)
    with _timed(("voxel_vote", N, C, max_points, M)):
        check(lib().orv_voxel_vote(_p(points), _p(point_coors), _p(order), _p(start), _p(seglen), _p(csum), N, C, int(max_points), int(M),
                                   _p(head_of), _p(out), _stream()), "orv_voxel_vote")
    return out


# ---- occupancy labelling and sparse Gaussian scene preparation (occupancy.hip) ----
def occ_project_labels(points, P, labels2d):
    """points fp32 [N,C], P fp32 [4,4] (intrin4 @ inverse(extrin), on the device), labels2d uint8 or int32 [H,W] -> labels int64 [N]."""
    _need_c(points, torch.float32, "points"), _need_c(P, torch.float32, "P")
    if labels2d.dtype not in (torch.uint8, torch.int32):
        raise RuntimeError(f"orv_amd.ops: `labels2d` must be torch.uint8 or torch.int32 (got {labels2d.dtype})")
    _need_c(labels2d, labels2d.dtype, "labels2d")
    _same_device((points, "points"), (P, "P"), (labels2d, "labels2d"))
    if points.dim() != 2 or tuple(P.shape) != (4, 4) or labels2d.dim() != 2:
        raise ValueError(f"occ_project_labels: points [N,C], P [4,4], labels2d [H,W] (got {tuple(points.shape)}, {tuple(P.shape)}, {tuple(labels2d.shape)})")
    N, C = points.shape
    H, W = labels2d.shape
    out = torch.empty(N, dtype=torch.int64, device=points.device)
    with _timed(("occ_project_labels", N, C, H, W)):
        check(lib().orv_occ_project_labels(_p(points), N, C, _p(P), _p(labels2d), labels2d.element_size(), H, W, _p(out), _stream()),
              "orv_occ_project_labels")
    return out


def occ_cell_keys(occ, grid, state):
    """occ int32 [M,4] = (x, y, z, label), grid = (X, Y, Z), state int64 [3] zeroed -> keys int64 [M]; state[1] is set by a row outside the grid."""
    _need_c(occ, torch.int32, "occ"), _need_c(state, torch.int64, "state")
    _same_device((occ, "occ"), (state, "state"))
    if occ.dim() != 2 or occ.shape[1] != 4 or state.numel() != 3:
        raise ValueError(f"occ_cell_keys: occ [M,4], state [3] (got {tuple(occ.shape)}, {tuple(state.shape)})")
    M = occ.shape[0]
    keys = torch.empty(M, dtype=torch.int64, device=occ.device)
    with _timed(("occ_cell_keys", M)):
        check(lib().orv_occ_cell_keys(_p(occ), M, int(grid[0]), int(grid[1]), int(grid[2]), _p(keys), _p(state), _stream()), "orv_occ_cell_keys")
    return keys


def occ_mark_cells(sorted_keys, order, occ, state):
    """-> last int32 [M]: 1 at the sorted entry that closes its cell; the clamped labels of those rows are ORed into state[0]."""
    _need_c(sorted_keys, torch.int64, "sorted_keys"), _need_c(order, torch.int64, "order"), _need_c(occ, torch.int32, "occ")
    _need_c(state, torch.int64, "state")
    _same_device((sorted_keys, "sorted_keys"), (order, "order"), (occ, "occ"), (state, "state"))
    M = sorted_keys.numel()
    if order.numel() != M or occ.numel() != 4 * M or state.numel() != 3:
        raise ValueError("occ_mark_cells: sorted_keys [M], order [M], occ [M,4], state [3]")
    last = torch.empty(M, dtype=torch.int32, device=occ.device)
    with _timed(("occ_mark_cells", M)):
        check(lib().orv_occ_mark_cells(_p(sorted_keys), _p(order), _p(occ), M, _p(last), _p(state), _stream()), "orv_occ_mark_cells")
    return last


def occ_write_gaussians(order, occ, last, csum, n, grid, axes, zscale, classes, num_channels):
    """-> (xyz [n,3], rgb [n,3], feat [n,F], rot [n,4], scale [n,3], opacity [n,1]) of the n surviving cells, in ascending order of the dense
    linear index; ``axes`` = the three fp32 coordinate tables, ``zscale`` the per-z scale table, ``classes`` the class bitmap."""
    _need_c(order, torch.int64, "order"), _need_c(occ, torch.int32, "occ")
    _need_c(last, torch.int32, "last"), _need_c(csum, torch.int32, "csum"), _need_c(zscale, torch.float32, "zscale")
    named = [(order, "order"), (occ, "occ"), (last, "last"), (csum, "csum"), (zscale, "zscale")]
    for t, name in zip(axes, ("axes[0]", "axes[1]", "axes[2]")):
        named.append((_need_c(t, torch.float32, name), name))
    _same_device(*named)
    M, (X, Y, Z), F = order.numel(), [int(g) for g in grid], int(num_channels)
    if occ.numel() != 4 * M or last.numel() != M or csum.numel() != M:
        raise ValueError("occ_write_gaussians: order / last / csum [M], occ [M,4]")
    if [t.numel() for t in axes] != [X, Y, Z] or zscale.numel() != Z:
        raise ValueError(f"occ_write_gaussians: the tables must hold {X}, {Y}, {Z} coordinates and {Z} scales")
    dev, f32 = occ.device, torch.float32
    n = int(n)
    xyz, rgb, scale = (torch.empty(max(n, 0), 3, dtype=f32, device=dev) for _ in range(3))
    feat, rot = torch.empty(max(n, 0), max(F, 0), dtype=f32, device=dev), torch.empty(max(n, 0), 4, dtype=f32, device=dev)
    opacity = torch.empty(max(n, 0), 1, dtype=f32, device=dev)
    with _timed(("occ_write_gaussians", M, n, F)):
        check(lib().orv_occ_write_gaussians(_p(order), _p(occ), _p(last), _p(csum), M, n, X, Y, Z, _p(axes[0]), _p(axes[1]),
                                            _p(axes[2]), _p(zscale), int(classes), F, _p(xyz), _p(rgb), _p(feat), _p(rot), _p(scale),
                                            _p(opacity), _stream()), "orv_occ_write_gaussians")
    return xyz, rgb, feat, rot, scale, opacity


# ---- control encoding: render arrays / uint8 frames -> the VAE encoder's input (conditions.hip) ----
COND_INTERP = {"nearest": 0, "bilinear": 1}
COND_POST = {None: 0, "none": 0, "depth": 1, "normalize": 2}
COND_OUT = {"nchw": 0, "vae": 1}


def cond_prepare(src, stages, interp, post=None, index=None, palette=None, out="nchw"):
    """src fp32 [N,h,w] (depth), uint8 [N,h,w] (label ids, with ``palette`` fp32 [P,3]) or uint8 [N,h,w,3] (RGB frames); ``stages`` = one or
    two (rh, rw, top, left, ch, cw); ``index`` int32 [n_out] = the source frame of every output frame (None: all, in order;
    an entry outside [0, N) gives a zero frame, ``orv_amd.conditions`` refuses it first) -> fp32 [n_out, C, H, W] (``out="nchw"``) or bf16 [n_out, H, W, 8] (``out="vae"``: channels 0-2 the data, 3-7 zero)."""
    if not isinstance(src, torch.Tensor):
        raise RuntimeError(f"orv_amd.ops: `src` must be a torch tensor on the GPU (got {type(src).__name__})")
    if src.dtype == torch.float32 and src.dim() == 3:
        kind = 0
    elif src.dtype == torch.uint8 and src.dim() == 3:
        kind = 1
    elif src.dtype == torch.uint8 and src.dim() == 4 and src.shape[3] == 3:
        kind = 2
    else:
        raise RuntimeError("orv_amd.ops: `src` must be torch.float32 [N,h,w], torch.uint8 [N,h,w] (label ids) or torch.uint8 [N,h,w,3] (RGB) "
                           f"(got {src.dtype} {tuple(src.shape)})")
    named = [(src, "src")]
    if (kind == 1) != (palette is not None):
        raise ValueError("orv_amd.ops: `palette` goes with uint8 label ids [N,h,w] and with nothing else")
    if palette is not None:
        if palette.dim() != 2 or palette.shape[1] != 3:
            raise ValueError(f"orv_amd.ops: `palette` must be [P,3] (got {tuple(palette.shape)})")
        named.append((palette, "palette"))
    if index is not None:
        if index.dim() != 1:
            raise ValueError(f"orv_amd.ops: `index` must be [n_out] (got {tuple(index.shape)})")
        named.append((index, "index"))
    for t, name in named:
        if t.requires_grad:
            raise RuntimeError(f"orv_amd.ops: `{name}` requires grad; cond_prepare has no backward (supported: tensors without grad)")
        _need_c(t, {"src": src.dtype, "palette": torch.float32, "index": torch.int32}[name], name)
    _same_device(*named)
    if interp not in COND_INTERP or post not in COND_POST or out not in COND_OUT:
        raise ValueError(f"orv_amd.ops: interp in {sorted(COND_INTERP)}, post in {[k for k in COND_POST if k]} or None, out in {sorted(COND_OUT)} "
                         f"(got {interp!r}, {post!r}, {out!r})")
    stages = [tuple(int(v) for v in s) for s in stages]
    if len(stages) not in (1, 2) or any(len(s) != 6 for s in stages):
        raise ValueError("orv_amd.ops: `stages` holds one or two (rh, rw, top, left, ch, cw)")
    flat = [v for s in stages for v in s]
    plan = (ctypes.c_int * len(flat))(*flat)
    N, h, w = src.shape[:3]
    n_out = N if index is None else index.numel()
    H, W = stages[-1][4], stages[-1][5]
    C = 1 if kind == 0 else 3
    if out == "nchw":
        res = torch.empty(n_out, C, max(H, 0), max(W, 0), dtype=torch.float32, device=src.device)
    else:
        res = torch.empty(n_out, max(H, 0), max(W, 0), 8, dtype=BF16, device=src.device)
    with _timed(("cond_prepare", kind, n_out, h, w, H, W, COND_OUT[out])):
        check(lib().orv_cond_prepare(_p(src), kind, N, h, w, _p(palette), 0 if palette is None else palette.shape[0], _p(index), n_out,
                                     plan, len(stages), COND_INTERP[interp], COND_POST[post], _p(res), COND_OUT[out], _stream()),
              "orv_cond_prepare")
    return res


# ---- video metrics (csrc/metrics.hip) ----
METRICS_SUPPORTED = "supported: torch.uint8 or torch.float32 GPU tensors of N frames x 3 channels, without grad"


def _frames_desc(t, name):
    """A [N, H, W, 3] view of any strides -> the orv_frames_t the kernel gathers through (no copy)."""
    from ._lib import Frames
    if not isinstance(t, torch.Tensor):
        raise RuntimeError(f"orv_amd.ops: `{name}` must be a torch tensor on the GPU (got {type(t).__name__}); {METRICS_SUPPORTED}")
    if not t.is_cuda:
        raise RuntimeError(f"orv_amd.ops: `{name}` must live on the GPU (got {t.device}); there is no CPU path; {METRICS_SUPPORTED}")
    if t.dtype not in (torch.uint8, torch.float32):
        raise RuntimeError(f"orv_amd.ops: `{name}` is {t.dtype}; {METRICS_SUPPORTED}")
    if t.requires_grad:
        raise RuntimeError(f"orv_amd.ops: `{name}` requires grad; frame_metrics has no backward; {METRICS_SUPPORTED}")
    if t.dim() != 4 or t.shape[3] != 3:
        raise ValueError(f"orv_amd.ops: `{name}` must be [N, H, W, 3] (a view of any strides) with 3 channels (got {tuple(t.shape)}); {METRICS_SUPPORTED}")
    storage = t.untyped_storage()
    f = Frames()
    f.data, f.kind, f.h, f.w = storage.data_ptr(), 0 if t.dtype == torch.float32 else 1, t.shape[1], t.shape[2]
    f.extent, f.offset = storage.nbytes() // t.element_size(), t.storage_offset()
    for k in range(4):
        f.stride[k] = t.stride(k)
    return f


def frame_metrics(pred, gt, size, data_range: float = 1.0, full: bool = False):
    """pred, gt: uint8 (divided by 255) or fp32 [N, H, W, 3] views of any strides, each with its own H and W; both are resized to
    ``size`` = (h, w) by the bilinear rule of DESIGN.md §16 -> fp64 [3, N] = (mse, psnr, ssim) per frame, and with ``full`` the fp32
    SSIM map [N, h - 6, w - 6, 3]."""
    fp, fg = _frames_desc(pred, "pred"), _frames_desc(gt, "gt")
    _same_device((pred, "pred"), (gt, "gt"))
    if pred.shape[0] != gt.shape[0]:
        raise ValueError(f"orv_amd.ops: `pred` has {pred.shape[0]} frames and `gt` has {gt.shape[0]}; supported: the same number of frames")
    h, w = (int(v) for v in size)
    if h < 7 or w < 7:
        raise ValueError(f"orv_amd.ops: size = {(h, w)}; supported: a resized height and width of at least 7 (one 7 x 7 window)")
    N = pred.shape[0]
    out = torch.empty(3, N, dtype=torch.float64, device=pred.device)
    ssim_map = torch.empty(N, h - 6, w - 6, 3, dtype=torch.float32, device=pred.device) if full else None
    nbytes = lib().orv_frame_metrics_workspace(N, h, w)
    ws = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=pred.device)
    with _timed(("frame_metrics", fp.kind, fg.kind, N, fp.h, fp.w, fg.h, fg.w, h, w, int(full))):
        check(lib().orv_frame_metrics(ctypes.byref(fp), ctypes.byref(fg), N, h, w, float(data_range), _p(out), _p(ssim_map), _p(ws), nbytes,
                                      _stream()), "orv_frame_metrics")
    return out, ssim_map


# ---- point-cloud cleaning and normals (csrc/pointcloud.hip) ----
def _pc_points(points, who):
    _need_c(points, torch.float32, "points")
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"{who}: points must be [N,3] (got {tuple(points.shape)})")
    return points.shape[0]


def _pc_grid(origin, cell, dims):
    return [float(v) for v in origin] + [float(cell)] + [int(g) for g in dims]


def pc_cells(points, origin, cell, dims):
    """-> keys int64 [N]: the linear key of every point's clamped cell on the grid ``origin`` [3] + ``cell`` * ``dims`` [3] (gx, gy, gz)."""
    N = _pc_points(points, "pc_cells")
    keys = torch.empty(N, dtype=torch.int64, device=points.device)
    with _timed(("pc_cells", N)):
        check(lib().orv_pc_cells(_p(points), N, *_pc_grid(origin, cell, dims), _p(keys), _stream()), "orv_pc_cells")
    return keys


def pc_cell_table(sorted_keys, order, points, n_cells):
    """-> (start int32 [n_cells + 1], sorted_points fp32 [N,3]) of the stably sorted keys; ``order`` = the sort's int64 indices."""
    N = _pc_points(points, "pc_cell_table")
    _need_c(sorted_keys, torch.int64, "sorted_keys"), _need_c(order, torch.int64, "order")
    _same_device((points, "points"), (sorted_keys, "sorted_keys"), (order, "order"))
    if sorted_keys.numel() != N or order.numel() != N:
        raise ValueError("pc_cell_table: sorted_keys [N], order [N], points [N,3]")
    start = torch.full((int(n_cells) + 1,), N, dtype=torch.int32, device=points.device)
    spts = torch.empty(N, 3, dtype=torch.float32, device=points.device)
    with _timed(("pc_cell_table", N, int(n_cells))):
        check(lib().orv_pc_cell_table(_p(sorted_keys), _p(order), _p(points), N, int(n_cells), _p(start), _p(spts), _stream()), "orv_pc_cell_table")
    return start, spts


def _pc_out(N, k, device):
    kk = min(int(k), N)
    return torch.empty(N, max(kk, 0), dtype=torch.int32, device=device), torch.empty(N, max(kk, 0), dtype=torch.float64, device=device)


def pc_knn(sorted_points, order, start, k, origin, cell, dims, out=None):
    """The grid walk -> (idx int32 [N, k'], d2 fp64 [N, k'], pending uint8 [N]); rows with pending = 1 are left to ``pc_knn_brute``."""
    N = _pc_points(sorted_points, "pc_knn")
    _need_c(order, torch.int64, "order"), _need_c(start, torch.int32, "start")
    _same_device((sorted_points, "sorted_points"), (order, "order"), (start, "start"))
    dims = [int(g) for g in dims]
    if order.numel() != N or start.numel() != dims[0] * dims[1] * dims[2] + 1:
        raise ValueError("pc_knn: sorted_points [N,3], order [N], start [gx * gy * gz + 1]")
    idx, d2 = out if out is not None else _pc_out(N, k, order.device)
    pending = torch.empty(N, dtype=torch.uint8, device=order.device)
    with _timed(("pc_knn", N, int(k), *dims)):
        check(lib().orv_pc_knn(_p(sorted_points), _p(order), _p(start), N, int(k), *_pc_grid(origin, cell, dims), _p(idx), _p(d2), _p(pending),
                               _stream()), "orv_pc_knn")
    return idx, d2, pending


def pc_knn_brute(points, k, queries, out=None):
    """The scan of all points for the int64 point numbers in ``queries`` [Q] -> (idx, d2) [N, k'] with those rows written (into ``out`` when given)."""
    N = _pc_points(points, "pc_knn_brute")
    _need_c(queries, torch.int64, "queries")
    _same_device((points, "points"), (queries, "queries"))
    idx, d2 = out if out is not None else _pc_out(N, k, points.device)
    _need_c(idx, torch.int32, "idx"), _need_c(d2, torch.float64, "d2")
    if idx.shape != (N, min(int(k), N)) or d2.shape != idx.shape:
        raise ValueError("pc_knn_brute: idx and d2 must be [N, min(k, N)]")
    with _timed(("pc_knn_brute", N, int(k), queries.numel())):
        check(lib().orv_pc_knn_brute(_p(points), N, int(k), _p(queries), queries.numel(), _p(idx), _p(d2), _stream()), "orv_pc_knn_brute")
    return idx, d2


def pc_outlier(d2, k, std_ratio):
    """d2 fp64 [N, k'] of a search with ``k`` -> (avg fp64 [N], stats fp64 [4] = mean, std, thr, V, keep uint8 [N])."""
    _need_c(d2, torch.float64, "d2")
    if d2.dim() != 2 or d2.shape[1] != min(int(k), d2.shape[0]):
        raise ValueError(f"pc_outlier: d2 must be [N, min(k, N)] (got {tuple(d2.shape)} at k = {k})")
    N, dev = d2.shape[0], d2.device
    avg, keep = torch.empty(N, dtype=torch.float64, device=dev), torch.empty(N, dtype=torch.uint8, device=dev)
    stats = torch.full((4,), float("nan"), dtype=torch.float64, device=dev)
    if N == 0:
        stats[3] = 0.0
    nbytes = lib().orv_pc_outlier_workspace(N)
    ws = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=dev)
    with _timed(("pc_outlier", N, int(k))):
        check(lib().orv_pc_outlier(_p(d2), N, int(k), float(std_ratio), _p(avg), _p(stats), _p(keep), _p(ws), nbytes, _stream()), "orv_pc_outlier")
    return avg, stats, keep


def pc_normals(points, idx, k, camera):
    """idx int32 [N, k'] of a search with ``k`` -> normals fp32 [N,3], oriented towards ``camera`` [3]."""
    N = _pc_points(points, "pc_normals")
    _need_c(idx, torch.int32, "idx")
    _same_device((points, "points"), (idx, "idx"))
    if idx.shape != (N, min(int(k), N)):
        raise ValueError(f"pc_normals: idx must be [N, min(k, N)] (got {tuple(idx.shape)} at k = {k})")
    normals = torch.empty(N, 3, dtype=torch.float32, device=points.device)
    with _timed(("pc_normals", N, int(k))):
        check(lib().orv_pc_normals(_p(points), _p(idx), N, int(k), *[float(c) for c in camera], _p(normals), _stream()), "orv_pc_normals")
    return normals


def pc_orient(points, normals, camera):
    """-> normals fp32 [N,3] turned towards ``camera`` [3]; a zero normal becomes the unit vector to the camera, or (0, 0, 1)."""
    N = _pc_points(points, "pc_orient")
    _need_c(normals, torch.float32, "normals")
    _same_device((points, "points"), (normals, "normals"))
    if normals.shape != points.shape:
        raise ValueError(f"pc_orient: normals must be [N,3] like points (got {tuple(normals.shape)})")
    out = torch.empty_like(normals)
    check(lib().orv_pc_orient(_p(points), _p(normals), N, *[float(c) for c in camera], _p(out), _stream()), "orv_pc_orient")
    return out


# ---- label-map compositing (csrc/labelmap.hip) ----
LM_DTYPES = {torch.bool: 1, torch.uint8: 1, torch.float32: 4}


def _lm_planes(masks, who):
    """masks [F,n,H,W] bool / uint8 / fp32 on the GPU whose inner [H,W] plane is contiguous -> (bytes per pixel, F, n, H, W, stride_f, stride_n)."""
    if not isinstance(masks, torch.Tensor) or masks.dtype not in LM_DTYPES:
        raise RuntimeError(f"orv_amd.ops: `masks` must be a torch.bool, torch.uint8 or torch.float32 tensor (got {getattr(masks, 'dtype', type(masks).__name__)})")
    _need(masks, masks.dtype, "masks")
    if masks.dim() != 4:
        raise ValueError(f"{who}: masks must be [F,n,H,W] (got {tuple(masks.shape)})")
    F, n, H, W = masks.shape
    if masks.numel() and ((W > 1 and masks.stride(3) != 1) or (H > 1 and masks.stride(2) != W)):
        raise ValueError(f"{who}: the inner [H,W] plane of `masks` must be contiguous (strides {masks.stride()})")
    return LM_DTYPES[masks.dtype], F, n, H, W, masks.stride(0) if F > 1 else 0, masks.stride(1) if n > 1 else 0


def lm_mask_stats(masks, threshold=0.0):
    """masks [F,n,H,W] -> (area int64 [F,n], xyxy int64 [F,n,4]): the count of set pixels and their inclusive box, zeros for an empty mask."""
    mb, F, n, H, W, sf, sn = _lm_planes(masks, "lm_mask_stats")
    dev = masks.device
    area, xyxy = torch.empty(F, n, dtype=torch.int64, device=dev), torch.empty(F, n, 4, dtype=torch.int64, device=dev)
    bands = min(max(H, 1), max(1, -(-1024 // max(F * n, 1))))          # about a thousand workgroups when the planes are few
    ws = torch.empty(max(F * n * bands * 5, 1), dtype=torch.int32, device=dev)
    with _timed(("lm_mask_stats", mb, F, n, H, W)):
        check(lib().orv_lm_mask_stats(_p(masks), mb, F, n, H, W, sf, sn, float(threshold), bands, _p(ws), _p(area), _p(xyxy), _stream()),
              "orv_lm_mask_stats")
    return area, xyxy


def lm_compose(masks, order, label_ids, palette, threshold=0.0):
    """masks [F,n,H,W]; ``order`` a sequence of m <= n mask numbers, ``label_ids`` n values in [0, 255], ``palette`` 60 triples in the
    channel order to be written (all on the host) -> (index uint8 [F,H,W], color uint8 [F,H,W,3])."""
    mb, F, n, H, W, sf, sn = _lm_planes(masks, "lm_compose")
    order, label_ids, palette = [int(j) for j in order], [int(v) for v in label_ids], [int(v) for t in palette for v in t]
    if len(label_ids) != n or any(not 0 <= v <= 255 for v in label_ids):
        raise ValueError(f"lm_compose: label_ids must hold n = {n} values in [0, 255]")
    if len(palette) != 180 or any(not 0 <= v <= 255 for v in palette):
        raise ValueError("lm_compose: palette must hold 60 triples of values in [0, 255]")
    m, dev = len(order), masks.device
    index, color = torch.empty(F, H, W, dtype=torch.uint8, device=dev), torch.empty(F, H, W, 3, dtype=torch.uint8, device=dev)
    steps = torch.empty(m + 256, dtype=torch.int32, device=dev)
    with _timed(("lm_compose", mb, F, n, m, H, W)):
        check(lib().orv_lm_compose(_p(masks), mb, F, n, H, W, sf, sn, float(threshold), (ctypes.c_int * max(m, 1))(*order), m,
                                   (ctypes.c_ubyte * max(n, 1))(*label_ids), (ctypes.c_ubyte * 180)(*palette), _p(steps), _p(index), _p(color),
                                   _stream()), "orv_lm_compose")
    return index, color


# ---- cascaded rollouts: the chunk boundary (csrc/frames.hip) ----
def _behind(t):
    """Elements of ``t``'s storage from its first element on: the extent the kernels' bound checks are held to."""
    return t.untyped_storage().nbytes() // t.element_size() - t.storage_offset()


def frames_quantize(video, f0: int = 0, f1: Optional[int] = None, out=None, dst_f0: int = 0):
    """video bf16 / fp32 [B, 3, F, H, W] (a view of any strides: the decoder's output) -> frames [f0, f1) of every clip as uint8
    [B, f1 - f0, H, W, 3], by ``postprocess_video``'s 'pil' arithmetic (x / 2 + 0.5, clamp, * 255, round half to even; NaN -> 0).  With
    ``out`` (uint8 [B, N, H, W, 3] whose frames are contiguous; batch and frame strides are free) they are written at frame offset
    ``dst_f0`` of it and ``out`` is returned."""
    if not isinstance(video, torch.Tensor) or video.dtype not in (BF16, torch.float32):
        raise RuntimeError(f"orv_amd.ops: `video` must be a torch.bfloat16 or torch.float32 tensor (got {getattr(video, 'dtype', type(video).__name__)})")
    _need(video, video.dtype, "video")
    if video.dim() != 5 or video.shape[1] != 3 or 0 in video.shape:
        raise ValueError(f"frames_quantize: video must be [B, 3, F, H, W] and not empty (got {tuple(video.shape)})")
    B, _, F, H, W = video.shape
    f1 = F if f1 is None else int(f1)
    f0, dst_f0 = int(f0), int(dst_f0)
    if not 0 <= f0 <= f1 <= F:
        raise ValueError(f"frames_quantize: frames [{f0}, {f1}) of a clip of {F}; supported: 0 <= f0 <= f1 <= F")
    if out is None:
        if dst_f0:
            raise ValueError("frames_quantize: dst_f0 needs `out`")
        out = torch.empty(B, f1 - f0, H, W, 3, dtype=torch.uint8, device=video.device)
    _need(out, torch.uint8, "out")
    _same_device((video, "video"), (out, "out"))
    if out.dim() != 5 or out.shape[0] != B or tuple(out.shape[2:]) != (H, W, 3):
        raise ValueError(f"frames_quantize: out must be [B = {B}, N, H = {H}, W = {W}, 3] (got {tuple(out.shape)})")
    if dst_f0 < 0 or dst_f0 + (f1 - f0) > out.shape[1]:
        raise ValueError(f"frames_quantize: {f1 - f0} frames at frame offset {dst_f0} of a destination of {out.shape[1]} frames")
    if out.numel() and tuple(out.stride()[2:]) != (W * 3, 3, 1):
        raise ValueError(f"frames_quantize: the [H, W, 3] frames of `out` must be contiguous (strides {out.stride()})")
    if f1 > f0:
        with _timed(("frames_quantize", video.element_size(), B, f1 - f0, H, W)):
            check(lib().orv_frames_quantize(_p(video), video.element_size(), _behind(video), (ctypes.c_long * 5)(*video.stride()), B, H, W, f0, f1,
                                            _p(out), _behind(out), out.stride(0), out.stride(1), dst_f0, _stream()), "orv_frames_quantize")
    return out


def frames_handoff(frames, index: int, table):
    """frames uint8 [B, F, H, W, 3] (a view of any strides), ``table`` bf16 [256] on the same device -> frame ``index`` of every clip as
    the bf16 channels-last tensor [B, 1, H, W, 8] that ``vae.encode_channels_last`` reads: channels 0-2 = table[level], 3-7 zero."""
    _need(frames, torch.uint8, "frames"), _need(table, BF16, "table")
    _same_device((frames, "frames"), (table, "table"))
    if frames.dim() != 5 or frames.shape[4] != 3 or 0 in frames.shape:
        raise ValueError(f"frames_handoff: frames must be [B, F, H, W, 3] and not empty (got {tuple(frames.shape)})")
    if tuple(table.shape) != (256,) or not table.is_contiguous():
        raise ValueError(f"frames_handoff: table must be a contiguous bf16 [256] (got {tuple(table.shape)})")
    B, F, H, W, _ = frames.shape
    index = int(index)
    if not 0 <= index < F:
        raise ValueError(f"frames_handoff: frame {index} of clips of {F} frames")
    out = torch.empty(B, 1, H, W, 8, dtype=BF16, device=frames.device)
    with _timed(("frames_handoff", B, H, W)):
        check(lib().orv_frames_handoff(_p(frames), _behind(frames), (ctypes.c_long * 5)(*frames.stride()), B, F, H, W, index, _p(table), _p(out),
                                       _stream()), "orv_frames_handoff")
    return out


# ---- first-block step cache (csrc/step_cache.hip) ----
def _sc_dense(named, B, Nv, D):
    for t, n in named:
        _need_c(t, BF16, n)
        if t.numel() != B * Nv * D:
            raise ValueError(f"orv_amd.ops: `{n}` must hold [B = {B}, Nv = {Nv}, D = {D}] values (got {tuple(t.shape)})")


def _sc_joint(x, B, Nt, Nv, D):
    _need_c(x, BF16, "x")
    if min(B, Nv, D) < 1 or Nt < 0 or x.numel() != B * (Nt + Nv) * D:
        raise ValueError(f"orv_amd.ops: `x` must be the joint buffer [B = {B}, Nt + Nv = {Nt} + {Nv}, D = {D}] (got {tuple(x.shape)})")


def step_cache_scratch(B: int, Nv: int, D: int) -> int:
    """Doubles of scratch ``step_cache_probe`` needs for this shape."""
    n = lib().orv_step_cache_scratch(B, Nv, D)
    if n < 0:
        check(1, "orv_step_cache_scratch")
    return int(n)


def step_cache_probe(x, e, p, f, c, sums, B, Nt, Nv, D, scratch=None):
    """x: the joint bf16 buffer [B, Nt + Nv, D] after iteration 0; e, p: dense bf16 [B, Nv, D] (embedding output, stored first residual).
    Writes f (dense copy of x's video rows), c = bf16(f - e) and ``sums`` fp64 [B, 2] = (sum |c - p|, sum |p|) per clip; -> sums."""
    _sc_joint(x, B, Nt, Nv, D)
    _sc_dense(((e, "e"), (p, "p"), (f, "f"), (c, "c")), B, Nv, D)
    _need_c(sums, torch.float64, "sums")
    if sums.numel() != 2 * B:
        raise ValueError(f"orv_amd.ops: `sums` must be fp64 [B = {B}, 2] (got {tuple(sums.shape)})")
    if scratch is None:
        scratch = torch.empty(step_cache_scratch(B, Nv, D), dtype=torch.float64, device=x.device)
    _need_c(scratch, torch.float64, "scratch")
    _same_device((x, "x"), (e, "e"), (p, "p"), (f, "f"), (c, "c"), (sums, "sums"), (scratch, "scratch"))
    with _timed(("step_cache_probe", B, Nv, D)):
        check(lib().orv_step_cache_probe(_p(x), _p(e), _p(p), _p(f), _p(c), _p(scratch), scratch.numel(), _p(sums), B, Nt, Nv, D, _stream()),
              "orv_step_cache_probe")
    return sums


def step_cache_store(x, f, c, t, p, B, Nt, Nv, D):
    """x: the joint buffer after the last iteration.  Writes t = bf16(x's video rows - f) and p = c."""
    _sc_joint(x, B, Nt, Nv, D)
    _sc_dense(((f, "f"), (c, "c"), (t, "t"), (p, "p")), B, Nv, D)
    _same_device((x, "x"), (f, "f"), (c, "c"), (t, "t"), (p, "p"))
    with _timed(("step_cache_store", B, Nv, D)):
        check(lib().orv_step_cache_store(_p(x), _p(f), _p(c), _p(t), _p(p), B, Nt, Nv, D, _stream()), "orv_step_cache_store")


def step_cache_apply(x, t, B, Nt, Nv, D):
    """The video rows of the joint buffer x become bf16(x + t), in place; -> x."""
    _sc_joint(x, B, Nt, Nv, D)
    _sc_dense(((t, "t"),), B, Nv, D)
    _same_device((x, "x"), (t, "t"))
    with _timed(("step_cache_apply", B, Nv, D)):
        check(lib().orv_step_cache_apply(_p(x), _p(t), B, Nt, Nv, D, _stream()), "orv_step_cache_apply")
    return x


# ---- training-state snapshot and checksums (csrc/snapshot.hip) ----
def snapshot_chunk_bytes() -> int:
    """Bytes per chunk of the snapshot kernels (an entry is processed in pieces of this size)."""
    return int(lib().orv_snapshot_chunk_bytes())


def _snapshot_call(fn, what, tensors, copies):
    """One table launch over ``tensors`` (``copies[i]``: the destination of entry i, or None to sum it only) -> int64 [n, 2] on the device:
    the u64 pairs (s1, s2), as bit patterns (torch has no arithmetic on uint64; ``sums_to_ints`` reads them)."""
    import numpy as np
    dev = tensors[0].device
    for i, (t, c) in enumerate(zip(tensors, copies)):
        for x, name in ((t, f"tensors[{i}]"), (c, f"copies[{i}]")):
            if x is None:
                continue
            if not x.is_cuda or x.device != dev:
                raise RuntimeError(f"orv_amd.ops: {what}: `{name}` must live on the GPU of the first tensor ({dev}; got {x.device}); there is no CPU path")
            if not x.is_contiguous():
                raise RuntimeError(f"orv_amd.ops: {what}: `{name}` must be contiguous")
            if x.data_ptr() % 4:
                raise RuntimeError(f"orv_amd.ops: {what}: `{name}` must start at a 4-byte aligned address")
    nbytes = [t.numel() * t.element_size() for t in tensors]
    n = len(tensors)
    table = np.zeros((n, 3), dtype=np.int64)
    table[:, 0] = [t.data_ptr() if b else 0 for t, b in zip(tensors, nbytes)]
    table[:, 1] = [c.data_ptr() if c is not None and b else 0 for c, b in zip(copies, nbytes)]
    table[:, 2] = nbytes
    host = torch.from_numpy(table).pin_memory()          # read by the library now (validation) and by the copy engine on the stream
    entries = host.to(dev, non_blocking=True)
    need = lib().orv_snapshot_scratch_bytes(n, int(sum(nbytes)))
    if need < 0:
        check(1, "orv_snapshot_scratch_bytes")
    scratch = torch.empty(int(need), dtype=torch.uint8, device=dev)
    sums = torch.empty((n, 2), dtype=torch.int64, device=dev)
    with _timed((what, n, int(sum(nbytes)))):
        check(fn(_p(entries), host.data_ptr(), n, _p(sums), _p(scratch), scratch.numel(), _stream()), what)
    return sums


def snapshot_into(tensors, copies):
    """``snapshot`` into destinations of the caller: ``copies[i]`` receives ``tensors[i]`` (None: summed only) and must hold as many bytes;
    any 4-byte aligned address is taken, independently of the source's.  -> ``sums``."""
    tensors, copies = list(tensors), list(copies)
    if len(tensors) != len(copies) or not tensors:
        raise ValueError(f"orv_amd.ops: snapshot_into: {len(copies)} destinations for {len(tensors)} tensors (at least one)")
    for i, (t, c) in enumerate(zip(tensors, copies)):
        if c is not None and c.numel() * c.element_size() != t.numel() * t.element_size():
            raise ValueError(f"orv_amd.ops: snapshot_into: `copies[{i}]` holds another number of bytes than `tensors[{i}]`")
    return _snapshot_call(lib().orv_snapshot, "orv_snapshot", tensors, copies)


def snapshot(tensors, copy=None):
    """Copy every tensor of the list into a new tensor and checksum it, all in one table launch plus one combine launch on the current stream
    (``orv_snapshot``) -> ``(copies, sums)``.  ``copy``: optional list of booleans; an entry with False is summed only and its copy is None.
    ``sums`` is int64 [n, 2] on the device (``sums_to_ints``).  Contiguous GPU tensors of any dtype, 4-byte aligned, on one device."""
    tensors = list(tensors)
    if not tensors:
        return [], torch.empty((0, 2), dtype=torch.int64)
    flags = [True] * len(tensors) if copy is None else [bool(c) for c in copy]
    if len(flags) != len(tensors):
        raise ValueError(f"orv_amd.ops: snapshot: {len(flags)} copy flags for {len(tensors)} tensors")
    copies = [torch.empty_like(t, memory_format=torch.contiguous_format) if f and t.is_cuda else None for t, f in zip(tensors, flags)]
    return copies, snapshot_into(tensors, copies)


def checksum(tensors):
    """``sums`` of ``snapshot`` without a copy (``orv_checksum``): nothing but the sums is written."""
    tensors = list(tensors)
    if not tensors:
        return torch.empty((0, 2), dtype=torch.int64)
    return _snapshot_call(lib().orv_checksum, "orv_checksum", tensors, [None] * len(tensors))


def sums_to_ints(sums):
    """int64 [n, 2] (device or host) -> list of (s1, s2) Python ints in [0, 2^64).  Synchronises with the stream that wrote ``sums``."""
    return [(int(a) & 0xFFFFFFFFFFFFFFFF, int(b) & 0xFFFFFFFFFFFFFFFF) for a, b in sums.cpu().tolist()]
