// Forward Gaussian rasterizer behind ORV's depth / semantic conditioning renders (the reference splats the occupied voxels through the
// CUDA extension orv/ops/diff-gaussian-rasterization, called by orv/dataset/gs_render.py:97-171 from orv/dataset/prepare_dataset.py:2023-2235).
// Written from the arithmetic contract in DESIGN.md §12, not from that extension's sources: projection + tile rectangle per Gaussian,
// one (tile | depth) key per covered tile, tile ranges from the sorted keys, and a per-tile front-to-back blend whose list is staged
// through LDS.  Forward only, fp32 throughout, no atomics: the result is bit-reproducible.
#include "common.hpp"

// The discrete decisions (near plane, radius, tile rectangle, the three blend thresholds) are specified on individually rounded fp32
// operations, so nothing in this file may be contracted into a fused multiply-add behind the source's back; the accumulations that may
// be fused say so with __builtin_fmaf.
#pragma clang fp contract(off)

namespace {

constexpr int GS_TILE = 16;          // pixels per tile edge; one 256-thread workgroup per tile
constexpr int GS_BATCH = 256;        // list entries staged per LDS batch
constexpr int GS_MAX_F = 16;
constexpr float GS_NEAR = 0.01f;
constexpr float GS_BIG = 1.0e9f;     // float -> int conversions are taken of min(max(v, -1e9), 1e9): exact in the defined range; a NaN (outside the contract) gives -1e9

__device__ __forceinline__ int gs_trunc(float v) { return (int)fminf(fmaxf(v, -GS_BIG), GS_BIG); }
__device__ __forceinline__ int gs_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

struct GsPreArgs {
    const float *means, *scales, *rots, *opac, *view, *proj;
    float *xy, *conic_op, *depth;
    int *radii, *rect, *tiles;
    int N, H, W;
    float tanfovx, tanfovy, scale_mod;
};

// one thread per Gaussian: steps 1-7 of the contract
__global__ __launch_bounds__(256) void gs_preprocess_kernel(const GsPreArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.N) return;
    float V[16], P[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) V[k] = a.view[k], P[k] = a.proj[k];
    int radius = 0, tiles = 0, x0 = 0, y0 = 0, x1 = 0, y1 = 0;
    float px = 0.0f, py = 0.0f, ca = 0.0f, cb = 0.0f, cc = 0.0f, zv = 0.0f;
    const float mx = a.means[3 * i], my = a.means[3 * i + 1], mz = a.means[3 * i + 2];
    // row vector [p, 1] @ M, M row-major
    const float tx0 = mx * V[0] + my * V[4] + mz * V[8] + V[12];
    const float ty0 = mx * V[1] + my * V[5] + mz * V[9] + V[13];
    const float tz = mx * V[2] + my * V[6] + mz * V[10] + V[14];
    zv = tz;
    if (tz > GS_NEAR) {
        const float hx = mx * P[0] + my * P[4] + mz * P[8] + P[12];
        const float hy = mx * P[1] + my * P[5] + mz * P[9] + P[13];
        const float hw = mx * P[3] + my * P[7] + mz * P[11] + P[15];
        const float w = 1.0f / (hw + 1e-7f);
        px = ((hx * w + 1.0f) * (float)a.W - 1.0f) / 2.0f;
        py = ((hy * w + 1.0f) * (float)a.H - 1.0f) / 2.0f;
        // Sigma = (R S)(R S)^T, R from the normalised quaternion (r, x, y, z)
        float qr = a.rots[4 * i], qx = a.rots[4 * i + 1], qy = a.rots[4 * i + 2], qz = a.rots[4 * i + 3];
        const float qn = sqrtf(qr * qr + qx * qx + qy * qy + qz * qz);
        qr = qr / qn, qx = qx / qn, qy = qy / qn, qz = qz / qn;
        const float R[9] = {1.0f - 2.0f * (qy * qy + qz * qz), 2.0f * (qx * qy - qr * qz), 2.0f * (qx * qz + qr * qy),
                            2.0f * (qx * qy + qr * qz), 1.0f - 2.0f * (qx * qx + qz * qz), 2.0f * (qy * qz - qr * qx),
                            2.0f * (qx * qz - qr * qy), 2.0f * (qy * qz + qr * qx), 1.0f - 2.0f * (qx * qx + qy * qy)};
        const float s[3] = {a.scale_mod * a.scales[3 * i], a.scale_mod * a.scales[3 * i + 1], a.scale_mod * a.scales[3 * i + 2]};
        float M[9], S3[9];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) M[3 * r + c] = R[3 * r + c] * s[c];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) S3[3 * r + c] = M[3 * r] * M[3 * c] + M[3 * r + 1] * M[3 * c + 1] + M[3 * r + 2] * M[3 * c + 2];
        // Jacobian of the projection at the clamped view-space point
        const float limx = 1.3f * a.tanfovx, limy = 1.3f * a.tanfovy;
        const float tx = fminf(limx, fmaxf(-limx, tx0 / tz)) * tz, ty = fminf(limy, fmaxf(-limy, ty0 / tz)) * tz;
        const float fx = (float)a.W / (2.0f * a.tanfovx), fy = (float)a.H / (2.0f * a.tanfovy);
        const float j00 = fx / tz, j02 = -(fx * tx) / (tz * tz), j11 = fy / tz, j12 = -(fy * ty) / (tz * tz);
        // T = J Rw, Rw[r][c] = V[4 c + r] (the rotation block of world-to-camera)
        float T0[3], T1[3], U0[3], U1[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            T0[c] = j00 * V[4 * c] + j02 * V[4 * c + 2];
            T1[c] = j11 * V[4 * c + 1] + j12 * V[4 * c + 2];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            U0[c] = T0[0] * S3[c] + T0[1] * S3[3 + c] + T0[2] * S3[6 + c];
            U1[c] = T1[0] * S3[c] + T1[1] * S3[3 + c] + T1[2] * S3[6 + c];
        }
        const float va = U0[0] * T0[0] + U0[1] * T0[1] + U0[2] * T0[2] + 0.3f;
        const float vb = U0[0] * T1[0] + U0[1] * T1[1] + U0[2] * T1[2];
        const float vc = U1[0] * T1[0] + U1[1] * T1[1] + U1[2] * T1[2] + 0.3f;
        const float det = va * vc - vb * vb;
        if (det != 0.0f) {
            ca = vc / det, cb = -vb / det, cc = va / det;
            const float mid = (va + vc) / 2.0f;
            const float lam = mid + sqrtf(fmaxf(0.1f, mid * mid - det));
            const int rad = gs_trunc(ceilf(3.0f * sqrtf(lam)));
            const int gx = (a.W + GS_TILE - 1) / GS_TILE, gy = (a.H + GS_TILE - 1) / GS_TILE;
            const float fr = (float)rad;
            x0 = gs_clampi(gs_trunc((px - fr) / 16.0f), 0, gx);
            y0 = gs_clampi(gs_trunc((py - fr) / 16.0f), 0, gy);
            x1 = gs_clampi(gs_trunc((px + fr + 15.0f) / 16.0f), 0, gx);
            y1 = gs_clampi(gs_trunc((py + fr + 15.0f) / 16.0f), 0, gy);
            if (x1 > x0 && y1 > y0) {
                tiles = (x1 - x0) * (y1 - y0);
                radius = rad;
            }
        }
    }
    a.xy[2 * i] = px, a.xy[2 * i + 1] = py;
    *(float4*)(a.conic_op + 4 * (long)i) = make_float4(ca, cb, cc, a.opac[i]);
    a.depth[i] = zv;
    a.radii[i] = radius;
    *(int4*)(a.rect + 4 * (long)i) = tiles ? make_int4(x0, y0, x1, y1) : make_int4(0, 0, 0, 0);
    a.tiles[i] = tiles;
}

// one thread per Gaussian: its (tile | depth bits) keys at [offsets[i-1], offsets[i]) of the pair list
__global__ __launch_bounds__(256) void gs_tile_keys_kernel(const int* __restrict__ rect, const float* __restrict__ depth,
                                                           const long* __restrict__ offsets, int N, int gx, long L,
                                                           long* __restrict__ keys, int* __restrict__ idx) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int4 r = *(const int4*)(rect + 4 * (long)i);
    long o = i ? offsets[i - 1] : 0;
    const long end = offsets[i];
    if (o < 0 || end > L || end - o != (long)(r.z - r.x) * (r.w - r.y)) return;   // offsets that are not the rectangles' prefix sum: write nothing
    const unsigned long zb = __float_as_uint(depth[i]);
    for (int y = r.y; y < r.w; ++y)
        for (int x = r.x; x < r.z; ++x, ++o) {
            keys[o] = (long)(((unsigned long)(unsigned)(y * gx + x) << 32) | zb);
            idx[o] = i;
        }
}

// [start, end) of every tile's run in the sorted keys; tiles without a run keep the caller's zeros
__global__ __launch_bounds__(256) void gs_tile_ranges_kernel(const long* __restrict__ keys, long L, int ntiles, int* __restrict__ ranges) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= L) return;
    const unsigned t = (unsigned)((unsigned long)keys[i] >> 32);
    if (t >= (unsigned)ntiles) return;
    const unsigned p = i ? (unsigned)((unsigned long)keys[i - 1] >> 32) : 0xffffffffu;
    if (p != t) {
        ranges[2 * t] = (int)i;
        if (i && p < (unsigned)ntiles) ranges[2 * p + 1] = (int)i;
    }
    if (i == L - 1) ranges[2 * t + 1] = (int)L;
}

struct GsRenderArgs {
    const int *ranges, *list;
    const float *xy, *conic_op, *depth, *colors, *feats, *bg;
    float *out_color, *out_feat, *out_depth, *out_alpha;
    int N, F, H, W, gx;
    long L;
};

// One workgroup per 16x16 tile, one pixel per thread.  The tile's depth-ordered list is consumed in batches of 256 entries that the 256
// threads stage into LDS (one entry each: centre, conic + opacity, depth, colour, FP >= F feature channels, the tail zero), so the blend loop
// reads LDS only, every lane the same address (a broadcast).  Barriers: every thread, in or out of the image, done or not, takes the same
// two per batch; the batch count comes from the tile's range; the only early exit is the workgroup-wide vote that every pixel is done.
template <int FP>
__global__ __launch_bounds__(256) void gs_render_kernel(const GsRenderArgs a) {
    __shared__ float4 s_g0[GS_BATCH];    // px, py, conic A, conic B
    __shared__ float4 s_g1[GS_BATCH];    // conic C, opacity, depth, red
    __shared__ float2 s_g2[GS_BATCH];    // green, blue
    __shared__ float4 s_f[FP ? GS_BATCH * (FP / 4) : 1];
    __shared__ int s_done[4];
    const int tid = threadIdx.x, tile = blockIdx.x;
    const int x = (tile % a.gx) * GS_TILE + (tid & 15), y = (tile / a.gx) * GS_TILE + (tid >> 4);
    const bool inside = x < a.W && y < a.H;
    const float fx = (float)x, fy = (float)y;
    long start = a.ranges[2 * tile], end = a.ranges[2 * tile + 1];
    start = start < 0 ? 0 : (start > a.L ? a.L : start);
    end = end < start ? start : (end > a.L ? a.L : end);
    const int nbatch = (int)((end - start + GS_BATCH - 1) / GS_BATCH);
    bool done = !inside;
    float T = 1.0f, C0 = 0.0f, C1 = 0.0f, C2 = 0.0f, D = 0.0f;
    float Fa[FP ? FP : 1];
#pragma unroll
    for (int k = 0; k < FP; ++k) Fa[k] = 0.0f;

    for (int b = 0; b < nbatch; ++b) {
        const bool wave_done = __all(done);
        if ((tid & 63) == 0) s_done[tid >> 6] = wave_done;
        __syncthreads();                 // also: every wave has left the previous batch's blend loop
        if (s_done[0] & s_done[1] & s_done[2] & s_done[3]) break;
        const long e = start + (long)b * GS_BATCH + tid;
        {
            float4 g0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), g1 = g0;
            float2 g2 = make_float2(0.0f, 0.0f);
            float f[FP ? FP : 1];
#pragma unroll
            for (int k = 0; k < FP; ++k) f[k] = 0.0f;
            if (e < end) {
                const unsigned id = (unsigned)a.list[e];
                if (id < (unsigned)a.N) {    // an index outside the arrays stages as a zero-opacity entry
                    const float4 co = *(const float4*)(a.conic_op + 4 * (long)id);
                    g0 = make_float4(a.xy[2 * (long)id], a.xy[2 * (long)id + 1], co.x, co.y);
                    g1 = make_float4(co.z, co.w, a.depth[id], a.colors[3 * (long)id]);
                    g2 = make_float2(a.colors[3 * (long)id + 1], a.colors[3 * (long)id + 2]);
#pragma unroll
                    for (int k = 0; k < FP; ++k)
                        if (k < a.F) f[k] = a.feats[(long)id * a.F + k];
                }
            }
            s_g0[tid] = g0, s_g1[tid] = g1, s_g2[tid] = g2;
#pragma unroll
            for (int k = 0; k < FP / 4; ++k) s_f[tid * (FP / 4) + k] = make_float4(f[4 * k], f[4 * k + 1], f[4 * k + 2], f[4 * k + 3]);
        }
        __syncthreads();
        const long left = end - (start + (long)b * GS_BATCH);
        const int cnt = left < GS_BATCH ? (int)left : GS_BATCH;
        if (!wave_done) {                // wave-uniform; no barrier inside.  (A per-entry __all(done) break here measured 8 % slower.)
            for (int j = 0; j < cnt; ++j) {
                if (done) continue;
                const float4 g0 = s_g0[j], g1 = s_g1[j];
                const float dx = g0.x - fx, dy = g0.y - fy;
                const float power = -0.5f * (g0.z * dx * dx + g1.x * dy * dy) - g0.w * dx * dy;
                if (power > 0.0f) continue;
                const float alpha = fminf(0.99f, g1.y * expf(power));
                if (alpha < 1.0f / 255.0f) continue;
                const float Tn = T * (1.0f - alpha);      // formed in fp32: the stop below is defined on this rounding
                if (Tn < 0.0001f) {
                    done = true;
                    continue;
                }
                const float w = alpha * T;
                const float2 g2 = s_g2[j];
                C0 = __builtin_fmaf(w, g1.w, C0), C1 = __builtin_fmaf(w, g2.x, C1), C2 = __builtin_fmaf(w, g2.y, C2);
                D = __builtin_fmaf(w, g1.z, D);
#pragma unroll
                for (int k = 0; k < FP / 4; ++k) {
                    const float4 f = s_f[j * (FP / 4) + k];
                    Fa[4 * k] = __builtin_fmaf(w, f.x, Fa[4 * k]), Fa[4 * k + 1] = __builtin_fmaf(w, f.y, Fa[4 * k + 1]);
                    Fa[4 * k + 2] = __builtin_fmaf(w, f.z, Fa[4 * k + 2]), Fa[4 * k + 3] = __builtin_fmaf(w, f.w, Fa[4 * k + 3]);
                }
                T = Tn;
            }
        }
    }
    if (inside) {
        const long hw = (long)a.H * a.W, pix = (long)y * a.W + x;
        a.out_color[pix] = C0 + T * a.bg[0];
        a.out_color[hw + pix] = C1 + T * a.bg[1];
        a.out_color[2 * hw + pix] = C2 + T * a.bg[2];
#pragma unroll
        for (int k = 0; k < FP; ++k)
            if (k < a.F) a.out_feat[k * hw + pix] = Fa[k];
        a.out_depth[pix] = D;
        a.out_alpha[pix] = 1.0f - T;
    }
}

inline long gs_tiles(int H, int W) { return (long)((H + GS_TILE - 1) / GS_TILE) * ((W + GS_TILE - 1) / GS_TILE); }

}  // namespace

extern "C" int orv_gs_preprocess(const float* means3D, const float* scales, const float* rotations, const float* opacities,
                                 const float* viewmatrix, const float* projmatrix, int N, int H, int W, float tanfovx, float tanfovy,
                                 float scale_modifier, float* xy, float* conic_opacity, float* depth, int* radii, int* rect,
                                 int* tiles_touched, void* stream) {
    ORV_REQUIRE(N >= 0, "orv_gs_preprocess: N must not be negative (got %d)", N);
    ORV_REQUIRE(H > 0 && W > 0, "orv_gs_preprocess: image height and width must be positive (got %d x %d)", H, W);
    ORV_REQUIRE(tanfovx > 0.0f && tanfovy > 0.0f, "orv_gs_preprocess: tanfovx and tanfovy must be positive");
    ORV_REQUIRE(viewmatrix && projmatrix, "orv_gs_preprocess: null pointer (viewmatrix / projmatrix)");
    if (N == 0) return ORV_OK;
    ORV_REQUIRE(means3D && scales && rotations && opacities, "orv_gs_preprocess: null pointer (means3D / scales / rotations / opacities)");
    ORV_REQUIRE(xy && conic_opacity && depth && radii && rect && tiles_touched, "orv_gs_preprocess: null pointer (an output buffer)");
    ORV_REQUIRE(orv_aligned(conic_opacity, 16) && orv_aligned(rect, 16), "orv_gs_preprocess: conic_opacity and rect must be 16-byte aligned");
    ORV_REQUIRE(gs_tiles(H, W) < (1L << 31), "orv_gs_preprocess: %d x %d has 2^31 tiles or more", H, W);
    GsPreArgs a;
    a.means = means3D, a.scales = scales, a.rots = rotations, a.opac = opacities, a.view = viewmatrix, a.proj = projmatrix;
    a.xy = xy, a.conic_op = conic_opacity, a.depth = depth, a.radii = radii, a.rect = rect, a.tiles = tiles_touched;
    a.N = N, a.H = H, a.W = W, a.tanfovx = tanfovx, a.tanfovy = tanfovy, a.scale_mod = scale_modifier;
    hipLaunchKernelGGL(gs_preprocess_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    return orv_check_launch("orv_gs_preprocess");
}

extern "C" int orv_gs_tile_keys(const int* rect, const float* depth, const long* offsets, int N, int H, int W, long L, long* keys,
                                int* gaussian_idx, void* stream) {
    ORV_REQUIRE(N >= 0, "orv_gs_tile_keys: N must not be negative (got %d)", N);
    ORV_REQUIRE(H > 0 && W > 0, "orv_gs_tile_keys: image height and width must be positive (got %d x %d)", H, W);
    ORV_REQUIRE(L >= 0 && L < (1L << 31), "orv_gs_tile_keys: the pair count L = %ld must be in [0, 2^31)", L);
    ORV_REQUIRE(gs_tiles(H, W) < (1L << 31), "orv_gs_tile_keys: %d x %d has 2^31 tiles or more", H, W);
    if (N == 0 || L == 0) return ORV_OK;
    ORV_REQUIRE(rect && depth && offsets && keys && gaussian_idx, "orv_gs_tile_keys: null pointer");
    ORV_REQUIRE(orv_aligned(rect, 16) && orv_aligned(offsets, 8) && orv_aligned(keys, 8), "orv_gs_tile_keys: rect must be 16-byte, offsets and keys 8-byte aligned");
    hipLaunchKernelGGL(gs_tile_keys_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rect, depth, offsets, N,
                       (W + GS_TILE - 1) / GS_TILE, L, keys, gaussian_idx);
    return orv_check_launch("orv_gs_tile_keys");
}

extern "C" int orv_gs_tile_ranges(const long* sorted_keys, long L, int H, int W, int* ranges, void* stream) {
    ORV_REQUIRE(H > 0 && W > 0, "orv_gs_tile_ranges: image height and width must be positive (got %d x %d)", H, W);
    ORV_REQUIRE(L >= 0 && L < (1L << 31), "orv_gs_tile_ranges: the pair count L = %ld must be in [0, 2^31)", L);
    ORV_REQUIRE(gs_tiles(H, W) < (1L << 31), "orv_gs_tile_ranges: %d x %d has 2^31 tiles or more", H, W);
    ORV_REQUIRE(ranges, "orv_gs_tile_ranges: null pointer (ranges)");
    if (L == 0) return ORV_OK;
    ORV_REQUIRE(sorted_keys, "orv_gs_tile_ranges: null pointer (sorted_keys)");
    ORV_REQUIRE(orv_aligned(sorted_keys, 8), "orv_gs_tile_ranges: sorted_keys must be 8-byte aligned");
    hipLaunchKernelGGL(gs_tile_ranges_kernel, dim3((unsigned)((L + 255) / 256)), dim3(256), 0, (hipStream_t)stream, sorted_keys, L,
                       (int)gs_tiles(H, W), ranges);
    return orv_check_launch("orv_gs_tile_ranges");
}

extern "C" int orv_gs_render(const int* ranges, const int* point_list, long L, const float* xy, const float* conic_opacity,
                             const float* depth, const float* colors, const float* features, int N, int F, const float* bg, int H,
                             int W, float* out_color, float* out_feature, float* out_depth, float* out_alpha, void* stream) {
    ORV_REQUIRE(N >= 0, "orv_gs_render: N must not be negative (got %d)", N);
    ORV_REQUIRE(H > 0 && W > 0, "orv_gs_render: image height and width must be positive (got %d x %d)", H, W);
    ORV_REQUIRE(F >= 0 && F <= GS_MAX_F, "orv_gs_render: F = %d feature channels; supported: 0 to %d", F, GS_MAX_F);
    ORV_REQUIRE(L >= 0 && L < (1L << 31), "orv_gs_render: the pair count L = %ld must be in [0, 2^31)", L);
    ORV_REQUIRE(gs_tiles(H, W) < (1L << 31), "orv_gs_render: %d x %d has 2^31 tiles or more", H, W);
    ORV_REQUIRE(ranges && bg && out_color && out_depth && out_alpha && (F == 0 || out_feature), "orv_gs_render: null pointer (ranges / bg / an output plane)");
    ORV_REQUIRE(L == 0 || (N > 0 && point_list && xy && conic_opacity && depth && colors && (F == 0 || features)),
                "orv_gs_render: null pointer (a per-Gaussian array) with L = %ld pairs", L);
    ORV_REQUIRE(orv_aligned(conic_opacity, 16), "orv_gs_render: conic_opacity must be 16-byte aligned");
    GsRenderArgs a;
    a.ranges = ranges, a.list = point_list, a.xy = xy, a.conic_op = conic_opacity, a.depth = depth, a.colors = colors, a.feats = features;
    a.bg = bg, a.out_color = out_color, a.out_feat = out_feature, a.out_depth = out_depth, a.out_alpha = out_alpha;
    a.N = N, a.F = F, a.H = H, a.W = W, a.gx = (W + GS_TILE - 1) / GS_TILE, a.L = L;
    const dim3 grid((unsigned)gs_tiles(H, W)), block(256);
    hipStream_t s = (hipStream_t)stream;
    switch ((F + 3) / 4) {
        case 0: hipLaunchKernelGGL(gs_render_kernel<0>, grid, block, 0, s, a); break;
        case 1: hipLaunchKernelGGL(gs_render_kernel<4>, grid, block, 0, s, a); break;
        case 2: hipLaunchKernelGGL(gs_render_kernel<8>, grid, block, 0, s, a); break;
        case 3: hipLaunchKernelGGL(gs_render_kernel<12>, grid, block, 0, s, a); break;
        default: hipLaunchKernelGGL(gs_render_kernel<16>, grid, block, 0, s, a); break;
    }
    return orv_check_launch("orv_gs_render");
}
