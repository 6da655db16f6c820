// Control encoding, preparation half: the render arrays (depth fp32, label ids uint8) or uint8 video frames -> the tensor the VAE
// encoder's first convolution reads.  Replaces the per-frame torchvision loop of orv/dataset/dataset.py:255-295 and :852-888 (two
// resizes and two centre crops per frame on the CPU, then clamp / palette / normalise) and the repeat, permute, pad and cast that
// follow it in orv/dataset/encode_dataset.py:801-916 and in AutoencoderKLCogVideoX.encode: one launch per tensor, one 16-byte store per
// output pixel.  Written from the arithmetic contract in DESIGN.md §15 (restated in include/orv_mi355.h).
//   * one workgroup of 256 threads owns a 16 x 16 tile of the final image, one thread per pixel, blockIdx.z = the output frame;
//   * a two-stage bilinear plan first computes the part of the cropped stage-1 image its tile's stage-2 taps reach into LDS (rounded to
//     fp32, which is what the contract makes stage 2 read), then resamples from LDS: the stage-1 image never goes to HBM;
//   * nearest composes the two index maps (bit-identical to resizing twice: every stage only copies) and paints the palette afterwards;
//   * the weights are computed in registers from the formula; no tables, no atomics, plain vector stores: bit-reproducible.
#include "common.hpp"

// The contract rounds every product and sum to fp32 on its own (the same reason as occupancy.hip): no contraction into an FMA anywhere in
// this file, the host-side span arithmetic included.
#pragma clang fp contract(off)

namespace {

constexpr int CP_TILE = 16;                    // final pixels per workgroup and axis
constexpr int CP_MAX_DOWN = 4;                 // largest supported downscale per axis and stage: at most 2 * 4 + 2 = 10 taps
// stage-1 pixels a tile's stage-2 taps can reach per axis: the centres of 16 outputs span 15 * scale, plus the support on both sides and
// the two roundings: 15 * 4 + 2 * 4 + 2 = 70.  The host walks every tile with the same cp_span and refuses a plan that needs more.
constexpr int CP_REGION = 72;

struct CpStage {
    int nh, nw;                                // input
    int rh, rw;                                // resized
    int top, left;                             // centre-crop offset into the resized image
    int ch, cw;                                // cropped = the stage's output
};

struct CpArgs {
    const void* src;
    const float* palette;
    const int* index;
    void* out;
    CpStage st[2];
    int n_stage, src_kind, interp, post, out_kind, N, n_out, n_palette;
};

// taps [lo, hi) of output i when n inputs are resized to o outputs, the centre c and the reciprocal scale the weights use
__host__ __device__ __forceinline__ void cp_span(int i, int n, int o, int& lo, int& hi, float& c, float& inv) {
    const float scale = (float)n / (float)o;
    const float support = scale >= 1.0f ? scale : 1.0f;
    inv = scale >= 1.0f ? 1.0f / scale : 1.0f;
    c = scale * ((float)i + 0.5f);
    const int a = (int)((c - support) + 0.5f), b = (int)((c + support) + 0.5f);
    lo = a > 0 ? a : 0;
    hi = b < n ? b : n;
}
__device__ __forceinline__ float cp_weight(int j, float c, float inv) {
    const float w = 1.0f - fabsf((((float)j - c) + 0.5f) * inv);
    return w > 0.0f ? w : 0.0f;
}
__host__ __device__ __forceinline__ int cp_nearest(int i, int n, int o) {
    const int s = (int)floorf((float)i * ((float)n / (float)o));
    return s < n - 1 ? s : n - 1;
}

// One antialiased-bilinear output at (y, x) of the resized image [oh, ow] from an [nh, nw] input read through fetch(row, col): the
// horizontal pass of every tap row first, rounded to fp32, then the vertical pass over those.
template <class F>
__device__ __forceinline__ float cp_resample(F fetch, int y, int x, int nh, int nw, int oh, int ow) {
    int ylo, yhi, xlo, xhi;
    float yc, yinv, xc, xinv;
    cp_span(y, nh, oh, ylo, yhi, yc, yinv);
    cp_span(x, nw, ow, xlo, xhi, xc, xinv);
    float xs = 0.0f, ys = 0.0f;
    for (int j = xlo; j < xhi; ++j) xs = xs + cp_weight(j, xc, xinv);
    for (int r = ylo; r < yhi; ++r) ys = ys + cp_weight(r, yc, yinv);
    float acc = 0.0f;
    for (int r = ylo; r < yhi; ++r) {
        float row = 0.0f;
        for (int j = xlo; j < xhi; ++j) row = row + fetch(r, j) * (cp_weight(j, xc, xinv) / xs);
        acc = acc + row * (cp_weight(r, yc, yinv) / ys);
    }
    return acc;
}

// channel c of source pixel (y, x) of frame f: fp32 as it is, uint8 RGB divided by 255
struct CpSource {
    const void* src;
    long frame;                                // element offset of the frame
    int w, kind, c;
    __device__ __forceinline__ float operator()(int y, int x) const {
        const long p = frame + (long)y * w + x;
        if (kind == ORV_COND_SRC_F32) return ((const float*)src)[p];
        return (float)((const unsigned char*)src)[frame * 3 + ((long)y * w + x) * 3 + c] / 255.0f;
    }
};
struct CpLds {
    const float* lds;
    int y0, x0, rw;
    __device__ __forceinline__ float operator()(int y, int x) const { return lds[(y - y0) * rw + (x - x0)]; }
};

__device__ __forceinline__ float cp_post(float v, int post) {
    if (post == ORV_COND_POST_DEPTH) {
        v = v < 0.01f ? 0.01f : (v > 0.4f ? 0.4f : v);          // a NaN stays a NaN, as in torch.clamp
        return v * 2.5f;
    }
    if (post == ORV_COND_POST_NORMALIZE) return (v - 0.5f) / 0.5f;
    return v;
}

__global__ __launch_bounds__(256) void cp_prepare_kernel(const CpArgs a) {
    __shared__ float region[CP_REGION * CP_REGION];
    const CpStage& last = a.st[a.n_stage - 1];
    const int tx = threadIdx.x & (CP_TILE - 1), ty = threadIdx.x >> 4;
    const int oy0 = blockIdx.y * CP_TILE, ox0 = blockIdx.x * CP_TILE;
    const int oy = oy0 + ty, ox = ox0 + tx, k = blockIdx.z;
    const int H = last.ch, W = last.cw;
    const bool live = oy < H && ox < W;
    const int C = a.src_kind == ORV_COND_SRC_F32 ? 1 : 3;
    int f = a.index ? a.index[k] : k;
    const bool known = (unsigned)f < (unsigned)a.N;             // the caller validates the list; an entry outside it reads nothing
    if (!known) f = 0;
    const CpStage& s0 = a.st[0];
    CpSource source{a.src, (long)f * s0.nh * s0.nw, s0.nw, a.src_kind, 0};
    float res[3] = {0.0f, 0.0f, 0.0f};

    if (a.interp == ORV_COND_NEAREST) {
        if (live) {
            int y = oy, x = ox;
            for (int s = a.n_stage - 1; s >= 0; --s) {
                y = cp_nearest(y + a.st[s].top, a.st[s].nh, a.st[s].rh);
                x = cp_nearest(x + a.st[s].left, a.st[s].nw, a.st[s].rw);
            }
            if (a.src_kind == ORV_COND_SRC_IDS) {
                int id = ((const unsigned char*)a.src)[source.frame + (long)y * s0.nw + x];
                id = id < a.n_palette ? id : a.n_palette - 1;
                for (int c = 0; c < 3; ++c) res[c] = a.palette[3 * id + c] / 255.0f;
            } else {
                for (int c = 0; c < C; ++c) {
                    source.c = c;
                    res[c] = source(y, x);
                }
            }
        }
    } else if (a.n_stage == 1) {
        if (live)
            for (int c = 0; c < C; ++c) {
                source.c = c;
                res[c] = cp_resample(source, oy + s0.top, ox + s0.left, s0.nh, s0.nw, s0.rh, s0.rw);
            }
    } else {
        // the block of the cropped stage-1 image [s0.ch, s0.cw] that this tile's stage-2 taps reach (the spans are monotone in the output)
        const int ty1 = (oy0 + CP_TILE < H ? oy0 + CP_TILE : H) - 1, tx1 = (ox0 + CP_TILE < W ? ox0 + CP_TILE : W) - 1;
        int ry0, ry1, rx0, rx1, unused;
        float fc, fi;
        cp_span(oy0 + last.top, last.nh, last.rh, ry0, unused, fc, fi);
        cp_span(ty1 + last.top, last.nh, last.rh, unused, ry1, fc, fi);
        cp_span(ox0 + last.left, last.nw, last.rw, rx0, unused, fc, fi);
        cp_span(tx1 + last.left, last.nw, last.rw, unused, rx1, fc, fi);
        int RH = ry1 - ry0, RW = rx1 - rx0;
        RH = RH < CP_REGION ? RH : CP_REGION;                   // never taken: the host refuses such a plan
        RW = RW < CP_REGION ? RW : CP_REGION;
        for (int c = 0; c < C; ++c) {
            source.c = c;
            for (int e = threadIdx.x; e < RH * RW; e += 256) {
                const int ry = e / RW, rx = e - ry * RW;
                region[e] = cp_resample(source, ry0 + ry + s0.top, rx0 + rx + s0.left, s0.nh, s0.nw, s0.rh, s0.rw);
            }
            __syncthreads();
            if (live) res[c] = cp_resample(CpLds{region, ry0, rx0, RW}, oy + last.top, ox + last.left, last.nh, last.nw, last.rh, last.rw);
            __syncthreads();
        }
    }
    if (!live) return;
    for (int c = 0; c < 3; ++c) res[c] = known ? cp_post(res[c], a.post) : 0.0f;
    if (a.out_kind == ORV_COND_OUT_NCHW) {
        float* o = (float*)a.out + ((long)k * C * H + oy) * W + ox;
        for (int c = 0; c < C; ++c) o[(long)c * H * W] = res[c];
    } else {
        if (C == 1) res[1] = res[2] = res[0];                   // depth repeated to three channels
        uint4 v;
        v.x = pack2bf(res[0], res[1]), v.y = pack2bf(res[2], 0.0f), v.z = 0u, v.w = 0u;
        *(uint4*)((bf16_t*)a.out + (((long)k * H + oy) * W + ox) * 8) = v;
    }
}

}  // namespace

extern "C" int orv_cond_prepare(const void* src, int src_kind, int N, int h, int w, const float* palette, int n_palette, const int* index,
                                int n_out, const int* plan, int n_stage, int interp, int post, void* out, int out_kind, void* stream) {
    const char* who = "orv_cond_prepare";
    ORV_REQUIRE(src_kind == ORV_COND_SRC_F32 || src_kind == ORV_COND_SRC_IDS || src_kind == ORV_COND_SRC_RGB8,
                "%s: src_kind = %d; supported: 0 (fp32 [N,h,w]), 1 (uint8 ids [N,h,w] with a palette), 2 (uint8 RGB [N,h,w,3])", who, src_kind);
    ORV_REQUIRE(interp == ORV_COND_NEAREST || interp == ORV_COND_BILINEAR, "%s: interp = %d; supported: 0 (nearest), 1 (antialiased bilinear)", who, interp);
    ORV_REQUIRE(post == ORV_COND_POST_NONE || post == ORV_COND_POST_DEPTH || post == ORV_COND_POST_NORMALIZE,
                "%s: post = %d; supported: 0 (none), 1 (depth: clamp to [0.01, 0.4], times 2.5), 2 (normalize: (x - 0.5) / 0.5)", who, post);
    ORV_REQUIRE(out_kind == ORV_COND_OUT_NCHW || out_kind == ORV_COND_OUT_VAE, "%s: out_kind = %d; supported: 0 (fp32 [n_out,C,H,W]), 1 (bf16 [n_out,H,W,8])", who, out_kind);
    ORV_REQUIRE(src_kind != ORV_COND_SRC_IDS || interp == ORV_COND_NEAREST, "%s: label ids are resized with nearest only (interp = 0)", who);
    ORV_REQUIRE(n_stage == 1 || n_stage == 2, "%s: n_stage = %d; supported: 1 or 2 stages of (resize, centre crop)", who, n_stage);
    ORV_REQUIRE(plan, "%s: null pointer (plan)", who);
    ORV_REQUIRE(N >= 1 && h >= 1 && w >= 1 && (long)N * h * w * 3 < 2147483648L, "%s: the source is %d x %d x %d; supported: N, h, w >= 1 and 3 N h w < 2^31", who, N, h, w);
    ORV_REQUIRE(n_out >= 0 && n_out <= 65535, "%s: n_out = %d output frames; supported: 0 to 65535", who, n_out);
    CpArgs a;
    int nh = h, nw = w;
    for (int s = 0; s < n_stage; ++s) {
        const int* p = plan + 6 * s;
        CpStage& st = a.st[s];
        st.nh = nh, st.nw = nw, st.rh = p[0], st.rw = p[1], st.top = p[2], st.left = p[3], st.ch = p[4], st.cw = p[5];
        ORV_REQUIRE(st.rh >= 1 && st.rw >= 1 && st.rh <= 32768 && st.rw <= 32768, "%s: stage %d resizes to %d x %d; supported: 1 to 32768 per axis", who, s + 1, st.rh, st.rw);
        ORV_REQUIRE(st.ch >= 1 && st.cw >= 1 && st.top >= 0 && st.left >= 0 && st.top + st.ch <= st.rh && st.left + st.cw <= st.rw,
                    "%s: stage %d crops %d x %d at (%d, %d) out of %d x %d; supported: a crop inside its input (no padding)", who, s + 1, st.ch, st.cw,
                    st.top, st.left, st.rh, st.rw);
        ORV_REQUIRE(nh <= CP_MAX_DOWN * st.rh && nw <= CP_MAX_DOWN * st.rw, "%s: stage %d resizes %d x %d to %d x %d; supported: at most %d x downscale per axis and stage",
                    who, s + 1, nh, nw, st.rh, st.rw, CP_MAX_DOWN);
        nh = st.ch, nw = st.cw;
    }
    if (n_stage == 1) a.st[1] = a.st[0];
    const int H = nh, W = nw, C = src_kind == ORV_COND_SRC_F32 ? 1 : 3;
    ORV_REQUIRE((long)n_out * C * H * W < 2147483648L * 4, "%s: the output holds %d x %d x %d x %d values; supported: below 2^33", who, n_out, C, H, W);
    if (n_stage == 2 && interp == ORV_COND_BILINEAR) {
        // what the kernel's LDS block has to hold, by the kernel's own arithmetic over every tile row and column
        const CpStage& l = a.st[1];
        for (int axis = 0; axis < 2; ++axis) {
            const int n = axis ? l.nw : l.nh, o = axis ? l.rw : l.rh, off = axis ? l.left : l.top, len = axis ? W : H;
            for (int t0 = 0; t0 < len; t0 += CP_TILE) {
                const int t1 = (t0 + CP_TILE < len ? t0 + CP_TILE : len) - 1;
                int lo, hi, unused;
                float c, inv;
                cp_span(t0 + off, n, o, lo, unused, c, inv);
                cp_span(t1 + off, n, o, unused, hi, c, inv);
                ORV_REQUIRE(hi - lo >= 1 && hi - lo <= CP_REGION, "%s: a tile of stage 2 reaches %d stage-1 pixels on one axis; supported: 1 to %d", who, hi - lo, CP_REGION);
            }
        }
    }
    if (n_out == 0) return ORV_OK;
    ORV_REQUIRE(src && out, "%s: null pointer (src / out)", who);
    ORV_REQUIRE(src_kind != ORV_COND_SRC_IDS || (palette && n_palette >= 1 && n_palette <= 256), "%s: label ids need a palette of 1 to 256 fp32 [n,3] entries (got %d)", who, n_palette);
    ORV_REQUIRE(((uintptr_t)out & 15) == 0 && (src_kind != ORV_COND_SRC_F32 || ((uintptr_t)src & 3) == 0) && ((uintptr_t)index & 3) == 0 && ((uintptr_t)palette & 3) == 0,
                "%s: out must be 16-byte, an fp32 src, index and palette 4-byte aligned", who);
    a.src = src, a.palette = palette, a.index = index, a.out = out;
    a.n_stage = n_stage, a.src_kind = src_kind, a.interp = interp, a.post = post, a.out_kind = out_kind, a.N = N, a.n_out = n_out, a.n_palette = n_palette;
    const dim3 grid((unsigned)((W + CP_TILE - 1) / CP_TILE), (unsigned)((H + CP_TILE - 1) / CP_TILE), (unsigned)n_out);
    ORV_REQUIRE(grid.y <= 65535, "%s: the final image is %d rows; supported: at most %d", who, H, 65535 * CP_TILE);
    hipLaunchKernelGGL(cp_prepare_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
    return orv_check_launch(who);
}
