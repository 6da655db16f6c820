// The chunk boundary of a cascaded rollout (orv_amd/rollout.py), on the device: what the reference does on the host between two denoise
// loops (orv/pipeline/evaluation_control_to_video.py:349-362 through VideoProcessor.postprocess_video / preprocess).
//   * quantize: the decoder's output [B, 3, F, H, W] (bf16 or fp32, any element strides) to uint8 frames [B, F_out, H, W, 3], frames
//     [f0, f1) of every clip written at a frame offset of the destination, so that a chunk's stitched range lands in the episode buffer.
//     A lane owns 8 consecutive pixels of a row: three 16-byte plane loads (bf16) and 24 output bytes as six dwords.
//   * handoff: one uint8 frame per clip to the bf16 channels-last tensor [B, 1, H, W, 8] the VAE encoder reads, through a 256-entry table
//     built on the host with preprocess' own statements.  A lane owns a pixel: three bytes in, one 16-byte store.
// Written from the contract in DESIGN.md §19.  No atomics, no LDS; every output value depends on one input value: bit-reproducible.
#include "common.hpp"

namespace {

constexpr long FR_MAX_STRIDE = 1L << 40;
constexpr int FR_MAX_DIM = 1 << 20;

// postprocess_video's 'pil' branch in fp32, one rounding per step: y = fl(fl(x / 2) + 0.5), clamp to [0, 1], rint_half_even(fl(y * 255)).
// x * 0.5f IS fl(x / 2) for every x (both are the correctly rounded value of the same real number), so nothing is approximated; the
// contraction of the product and the sum into one FMA is switched off all the same.  fmaxf returns its other operand for a NaN: NaN -> 0.
__device__ __forceinline__ unsigned fr_q8(float x) {
#pragma clang fp contract(off)
    float y = x * 0.5f;
    y = y + 0.5f;
    y = fminf(fmaxf(y, 0.0f), 1.0f);
    return (unsigned)(int)rintf(y * 255.0f);
}

template <int SB> __device__ __forceinline__ float fr_load(const unsigned char* p, long i) {
    if (SB == 2) return bf2f(((const bf16_t*)p)[i]);
    return ((const float*)p)[i];
}
// 8 consecutive pixels of one plane, 16-byte aligned
template <int SB> __device__ __forceinline__ void fr_load8(const unsigned char* p, int g, float* v) {
    if (SB == 2) {
        const uint4 u = ((const uint4*)p)[g];
        const unsigned w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) v[2 * k] = __uint_as_float(w[k] << 16), v[2 * k + 1] = __uint_as_float(w[k] & 0xffff0000u);
    } else {
        const float4 a = ((const float4*)p)[2 * g], b = ((const float4*)p)[2 * g + 1];
        v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
    }
}

// The grid is sized over rows: 1 << shift lanes work on one row (the power of two at or above its W / 8 groups, at most 256), so a
// workgroup takes 256 >> shift rows.  A row goes through the vector path when x is the unit stride, its three plane rows start on
// 16-byte boundaries and its destination row on a 4-byte one; the last W % 8 pixels, and every pixel of any other row, go one at a time.
template <int SB>
__global__ __launch_bounds__(256) void frames_quantize_kernel(const unsigned char* __restrict__ src, long sb, long sc, long sf, long sy, long sx, int nf,
                                                              int H, int W, int f0, long rows, int shift, unsigned char* __restrict__ dst, long dsb,
                                                              long dsf, int dst_f0) {
    const long row = (long)blockIdx.x * (256 >> shift) + (threadIdx.x >> shift);
    if (row >= rows) return;
    const int lanes = 1 << shift, lane = threadIdx.x & (lanes - 1);
    const long t = row / H;
    const int y = (int)(row - t * H);
    const long b = t / nf;
    const int f = (int)(t - b * nf);
    const unsigned char* p[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) p[c] = src + (b * sb + c * sc + (long)(f0 + f) * sf + (long)y * sy) * SB;
    unsigned char* d = dst + b * dsb + (long)(dst_f0 + f) * dsf + (long)y * W * 3;
    const bool vec = sx == 1 && ((((uintptr_t)p[0] | (uintptr_t)p[1] | (uintptr_t)p[2]) & 15) == 0) && (((uintptr_t)d & 3) == 0);
    const int groups = vec ? W >> 3 : 0;
    for (int g = lane; g < groups; g += lanes) {
        float v[3][8];
#pragma unroll
        for (int c = 0; c < 3; ++c) fr_load8<SB>(p[c], g, v[c]);
        unsigned q[24];
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int c = 0; c < 3; ++c) q[3 * i + c] = fr_q8(v[c][i]);
        unsigned* o = (unsigned*)(d + (long)g * 24);
#pragma unroll
        for (int k = 0; k < 6; ++k) o[k] = q[4 * k] | q[4 * k + 1] << 8 | q[4 * k + 2] << 16 | q[4 * k + 3] << 24;
    }
    for (int x = groups * 8 + lane; x < W; x += lanes) {
#pragma unroll
        for (int c = 0; c < 3; ++c) d[(long)x * 3 + c] = (unsigned char)fr_q8(fr_load<SB>(p[c], (long)x * sx));
    }
}

__global__ __launch_bounds__(256) void frames_handoff_kernel(const unsigned char* __restrict__ src, long sb, long sy, long sx, long sc, int H, int W,
                                                             long total, const bf16_t* __restrict__ table, uint4* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long t = i / W;
    const int x = (int)(i - t * W);
    const long b = t / H;
    const int y = (int)(t - b * H);
    const unsigned char* p = src + b * sb + (long)y * sy + (long)x * sx;
    const unsigned r = table[p[0]], g = table[p[sc]], bl = table[p[2 * sc]];
    out[i] = make_uint4(r | g << 16, bl, 0u, 0u);                          // channels 3-7: zero
}

bool fr_strides_ok(const long* s, int n) {
    for (int k = 0; k < n; ++k)
        if (s[k] < 0 || s[k] >= FR_MAX_STRIDE) return false;
    return true;
}

}  // namespace

extern "C" int orv_frames_quantize(const void* src, int src_bytes, long src_extent, const long* src_stride, int B, int H, int W, int f0, int f1,
                                   unsigned char* dst, long dst_extent, long dst_stride_b, long dst_stride_f, int dst_f0, void* stream) {
    ORV_REQUIRE(src_bytes == 2 || src_bytes == 4, "orv_frames_quantize: src_bytes = %d; supported: 2 (bf16) or 4 (fp32)", src_bytes);
    ORV_REQUIRE(src && dst && src_stride, "orv_frames_quantize: null pointer (src / src_stride / dst)");
    ORV_REQUIRE(B >= 1 && H >= 1 && W >= 1 && B <= FR_MAX_DIM && H <= FR_MAX_DIM && W <= FR_MAX_DIM,
                "orv_frames_quantize: B = %d, H = %d, W = %d; supported: 1 to %d each", B, H, W, FR_MAX_DIM);
    ORV_REQUIRE(f0 >= 0 && f1 >= f0 && f1 <= FR_MAX_DIM && dst_f0 >= 0 && dst_f0 <= FR_MAX_DIM,
                "orv_frames_quantize: frames [%d, %d) to frame offset %d; supported: 0 <= f0 <= f1 <= %d, 0 <= dst_f0 <= %d", f0, f1, dst_f0,
                FR_MAX_DIM, FR_MAX_DIM);
    ORV_REQUIRE(fr_strides_ok(src_stride, 5), "orv_frames_quantize: source strides (b, c, f, y, x) must lie in [0, 2^40) elements");
    ORV_REQUIRE(orv_aligned(src, (uintptr_t)src_bytes), "orv_frames_quantize: src must be aligned to its element size (%d bytes)", src_bytes);
    const int nf = f1 - f0;
    if (nf == 0) return ORV_OK;
    const long src_last = (long)(B - 1) * src_stride[0] + 2 * src_stride[1] + (long)(f1 - 1) * src_stride[2] + (long)(H - 1) * src_stride[3] +
                          (long)(W - 1) * src_stride[4];
    ORV_REQUIRE(src_last < src_extent, "orv_frames_quantize: the last source element read is %ld and the buffer holds %ld", src_last, src_extent);
    const long frame_bytes = (long)H * W * 3;
    ORV_REQUIRE(dst_stride_f >= frame_bytes && dst_stride_f < FR_MAX_STRIDE && dst_stride_b >= 0 && dst_stride_b < FR_MAX_STRIDE &&
                    (B == 1 || dst_stride_b >= (long)nf * dst_stride_f),
                "orv_frames_quantize: destination strides (b = %ld, f = %ld bytes); supported: f >= H W 3 = %ld, b >= (f1 - f0) f when B > 1 "
                "(frames and clips do not overlap), both below 2^40", dst_stride_b, dst_stride_f, frame_bytes);
    const long dst_end = (long)(B - 1) * dst_stride_b + (long)(dst_f0 + nf - 1) * dst_stride_f + frame_bytes;
    ORV_REQUIRE(dst_end <= dst_extent, "orv_frames_quantize: the last byte written is %ld and the destination holds %ld", dst_end - 1, dst_extent);
    int shift = 0;
    while (shift < 8 && (1 << shift) < (W + 7) / 8) ++shift;
    const long rows = (long)B * nf * H;
    const long blocks = (rows + (256 >> shift) - 1) / (256 >> shift);
    ORV_REQUIRE(blocks <= 0x7fffffffL, "orv_frames_quantize: %ld rows need %ld workgroups; supported: at most 2^31 - 1", rows, blocks);
    const unsigned char* s = (const unsigned char*)src;
    hipStream_t st = (hipStream_t)stream;
    if (src_bytes == 2)
        frames_quantize_kernel<2><<<dim3((unsigned)blocks), dim3(256), 0, st>>>(s, src_stride[0], src_stride[1], src_stride[2], src_stride[3], src_stride[4],
                                                                                nf, H, W, f0, rows, shift, dst, dst_stride_b, dst_stride_f, dst_f0);
    else
        frames_quantize_kernel<4><<<dim3((unsigned)blocks), dim3(256), 0, st>>>(s, src_stride[0], src_stride[1], src_stride[2], src_stride[3], src_stride[4],
                                                                                nf, H, W, f0, rows, shift, dst, dst_stride_b, dst_stride_f, dst_f0);
    return orv_check_launch("orv_frames_quantize");
}

extern "C" int orv_frames_handoff(const unsigned char* src, long src_extent, const long* src_stride, int B, int F, int H, int W, int frame,
                                  const void* table, void* out, void* stream) {
    ORV_REQUIRE(src && src_stride && table && out, "orv_frames_handoff: null pointer (src / src_stride / table / out)");
    ORV_REQUIRE(B >= 1 && F >= 1 && H >= 1 && W >= 1 && B <= FR_MAX_DIM && F <= FR_MAX_DIM && H <= FR_MAX_DIM && W <= FR_MAX_DIM,
                "orv_frames_handoff: B = %d, F = %d, H = %d, W = %d; supported: 1 to %d each", B, F, H, W, FR_MAX_DIM);
    ORV_REQUIRE(frame >= 0 && frame < F, "orv_frames_handoff: frame = %d; supported: 0 to F - 1 = %d", frame, F - 1);
    ORV_REQUIRE(fr_strides_ok(src_stride, 5), "orv_frames_handoff: source strides (b, f, y, x, c) must lie in [0, 2^40) bytes");
    ORV_REQUIRE(orv_aligned(table, 2) && orv_aligned(out, 16), "orv_frames_handoff: table must be 2-byte and out 16-byte aligned");
    const long first = (long)frame * src_stride[1];
    const long last = first + (long)(B - 1) * src_stride[0] + (long)(H - 1) * src_stride[2] + (long)(W - 1) * src_stride[3] + 2 * src_stride[4];
    ORV_REQUIRE(last < src_extent, "orv_frames_handoff: the last source byte read is %ld and the buffer holds %ld", last, src_extent);
    const long total = (long)B * H * W;
    const long blocks = (total + 255) / 256;
    ORV_REQUIRE(blocks <= 0x7fffffffL, "orv_frames_handoff: %ld pixels need %ld workgroups; supported: at most 2^31 - 1", total, blocks);
    frames_handoff_kernel<<<dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream>>>(src + first, src_stride[0], src_stride[2], src_stride[3],
                                                                                        src_stride[4], H, W, total, (const bf16_t*)table, (uint4*)out);
    return orv_check_launch("orv_frames_handoff");
}
