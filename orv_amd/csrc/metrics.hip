// PSNR / SSIM of a generated clip against its ground truth, per frame, on frames already on the device.  Replaces the per-frame CPU loop
// of orv/pipeline/compute_metrics.py:38-80: cv2.resize(..., (320, 256), INTER_LINEAR) of both images, then skimage's
// peak_signal_noise_ratio and structural_similarity(channel_axis=-1, data_range=1.), spread over 64 threads.  Written from the arithmetic
// contract in DESIGN.md §16 (restated in include/orv_mi355.h).  Two launches per call:
//   * frame_metrics_kernel, grid (tiles of the resized image) x (frames): one workgroup of 256 threads owns a 32 x 32 block of resized
//     pixels and also resamples the 3-pixel halo around it, both images, three channels, into LDS (fp32; the resized images never go to
//     HBM); squared error of the owned pixels; per channel the separable 7-tap sums of a, b, a*a, b*b, a*b through LDS; S at every owned
//     pixel whose whole window lies inside the image (optionally stored); one record of four fp64 sums per (frame, tile);
//   * frame_metrics_finish_kernel, one wave per frame: the tile records summed in a fixed order, then mse, psnr and ssim.
// No atomics on floating-point data, every reduction in a fixed order: bit-reproducible.  Source reads are strided gathers (2 x 2 taps
// per resized pixel) through element strides for (n, y, x, c), so uint8 / fp32 NHWC, fp32 NCHW and width slices need no copy.
#include "common.hpp"

// The contract rounds every product and sum on its own (fp32 for the images, fp64 for the sample coordinate): no contraction into an FMA
// anywhere in this file.
#pragma clang fp contract(off)

namespace {

constexpr int FM_TILE = 32;                    // resized pixels a workgroup owns per axis
constexpr int FM_HALO = 3;                     // half of the 7-tap window
constexpr int FM_REGION = FM_TILE + 2 * FM_HALO;
constexpr int FM_REC = 4;                      // fp64 per (frame, tile): squared error, sum of S for channels 0, 1, 2

struct FmSource {
    const void* data;                          // the base pointer with the element offset already applied
    long sn, sy, sx, sc;                       // element strides
    int kind, h, w;
};

struct FmArgs {
    FmSource src[2];                           // prediction, ground truth
    double* records;
    float* ssim_map;                           // [N, h - 6, w - 6, 3] or null
    int N, h, w, tiles_x, n_tiles;
    float c1, c2;
};

// channel c of source pixel (y, x) of frame n: fp32 as it is, uint8 divided by 255
__device__ __forceinline__ float fm_fetch(const FmSource& s, long frame, int y, int x, int c) {
    const long p = frame + (long)y * s.sy + (long)x * s.sx + (long)c * s.sc;
    if (s.kind == ORV_METRICS_SRC_F32) return ((const float*)s.data)[p];
    return (float)((const unsigned char*)s.data)[p] / 255.0f;
}

// the two taps and the weight of output i when n inputs are resized to o outputs (cv2's INTER_LINEAR for float images)
__device__ __forceinline__ void fm_tap(int i, int n, int o, int& s, float& w) {
    const double scale = 1.0 / ((double)o / (double)n);
    const float f = (float)(((double)i + 0.5) * scale - 0.5);
    const float fl = floorf(f);
    s = (int)fl;
    w = f - fl;
    if (s < 0) s = 0, w = 0.0f;
    if (s >= n - 1) s = n - 1, w = 0.0f;
}

__device__ __forceinline__ double fm_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(256) void frame_metrics_kernel(const FmArgs a) {
    __shared__ float img[2][3][FM_REGION * FM_REGION];          // resized a (prediction) and b (ground truth), block + halo
    __shared__ float hsum[5][FM_REGION * FM_TILE];              // horizontal 7-tap sums of a, b, a*a, b*b, a*b for one channel
    __shared__ int tap_s[2][2][FM_REGION];                      // [image][axis: 0 = y, 1 = x][region row or column]
    __shared__ float tap_w[2][2][FM_REGION];
    __shared__ double red[4][FM_REC];

    const int tile = blockIdx.x, n = blockIdx.y;
    const int y0 = (tile / a.tiles_x) * FM_TILE, x0 = (tile % a.tiles_x) * FM_TILE;
    const int t = threadIdx.x;

    // the taps of every row and column of the region, once per workgroup (the fp64 coordinate arithmetic stays out of the pixel loop)
    if (t < 4 * FM_REGION) {
        const int which = t / FM_REGION, r = t - which * FM_REGION, im = which >> 1, axis = which & 1;
        const int g = (axis ? x0 : y0) - FM_HALO + r, o = axis ? a.w : a.h, nn = axis ? a.src[im].w : a.src[im].h;
        int s = 0;
        float w = 0.0f;
        if (g >= 0 && g < o) fm_tap(g, nn, o, s, w);
        tap_s[im][axis][r] = s, tap_w[im][axis][r] = w;
    }
    __syncthreads();

    // step 1: both images, three channels, block + halo -> LDS; a position outside the resized image holds zero and is never part of a
    // window that is evaluated
    for (int e = t; e < FM_REGION * FM_REGION; e += 256) {
        const int ry = e / FM_REGION, rx = e - ry * FM_REGION;
        const int gy = y0 - FM_HALO + ry, gx = x0 - FM_HALO + rx;
        const bool in = gy >= 0 && gy < a.h && gx >= 0 && gx < a.w;
#pragma unroll
        for (int im = 0; im < 2; ++im) {
            const FmSource& s = a.src[im];
            const int sy = tap_s[im][0][ry], sx = tap_s[im][1][rx];
            const int sy1 = sy + 1 < s.h ? sy + 1 : s.h - 1, sx1 = sx + 1 < s.w ? sx + 1 : s.w - 1;
            const float wy = tap_w[im][0][ry], wx = tap_w[im][1][rx];
            const long frame = (long)n * s.sn;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float v = 0.0f;
                if (in) {
                    const float top = fm_fetch(s, frame, sy, sx, c) * (1.0f - wx) + fm_fetch(s, frame, sy, sx1, c) * wx;
                    const float bot = fm_fetch(s, frame, sy1, sx, c) * (1.0f - wx) + fm_fetch(s, frame, sy1, sx1, c) * wx;
                    v = top * (1.0f - wy) + bot * wy;
                }
                img[im][c][e] = v;
            }
        }
    }
    __syncthreads();

    double acc[FM_REC] = {0.0, 0.0, 0.0, 0.0};
    const float cn = (float)(49.0 / 48.0);
    for (int c = 0; c < 3; ++c) {
        const float* A = img[0][c];
        const float* B = img[1][c];
        // step 3a: horizontal sums, seven terms left to right; entry (r, j) covers region columns j .. j + 6 of region row r
        for (int e = t; e < FM_REGION * FM_TILE; e += 256) {
            const int r = e / FM_TILE, j = e - r * FM_TILE;
            const float* pa = A + r * FM_REGION + j;
            const float* pb = B + r * FM_REGION + j;
            float sa = pa[0], sb = pb[0], saa = pa[0] * pa[0], sbb = pb[0] * pb[0], sab = pa[0] * pb[0];
#pragma unroll
            for (int k = 1; k < 7; ++k) {
                const float va = pa[k], vb = pb[k];
                sa = sa + va, sb = sb + vb, saa = saa + va * va, sbb = sbb + vb * vb, sab = sab + va * vb;
            }
            hsum[0][e] = sa, hsum[1][e] = sb, hsum[2][e] = saa, hsum[3][e] = sbb, hsum[4][e] = sab;
        }
        __syncthreads();
        // steps 2 and 3b-4: the owned pixels, four per thread
        for (int p = t; p < FM_TILE * FM_TILE; p += 256) {
            const int py = p / FM_TILE, px = p - py * FM_TILE;
            const int gy = y0 + py, gx = x0 + px;
            if (gy >= a.h || gx >= a.w) continue;
            const int centre = (py + FM_HALO) * FM_REGION + px + FM_HALO;
            const float d = A[centre] - B[centre];
            acc[0] += (double)(d * d);
            if (gy < FM_HALO || gy >= a.h - FM_HALO || gx < FM_HALO || gx >= a.w - FM_HALO) continue;
            float u[5];
#pragma unroll
            for (int q = 0; q < 5; ++q) {
                const float* col = hsum[q] + py * FM_TILE + px;          // rows py .. py + 6 = resized rows gy - 3 .. gy + 3
                float s = col[0];
#pragma unroll
                for (int k = 1; k < 7; ++k) s = s + col[k * FM_TILE];
                u[q] = s / 49.0f;
            }
            const float ux = u[0], uy = u[1];
            const float vx = cn * (u[2] - ux * ux), vy = cn * (u[3] - uy * uy), vxy = cn * (u[4] - ux * uy);
            const float a1 = 2.0f * ux * uy + a.c1, a2 = 2.0f * vxy + a.c2;
            const float b1 = ux * ux + uy * uy + a.c1, b2 = vx + vy + a.c2;
            const float S = (a1 * a2) / (b1 * b2);
            acc[1 + c] += (double)S;
            if (a.ssim_map)
                a.ssim_map[(((long)n * (a.h - 2 * FM_HALO) + (gy - FM_HALO)) * (a.w - 2 * FM_HALO) + (gx - FM_HALO)) * 3 + c] = S;
        }
        __syncthreads();
    }

    // steps 5-6: lanes by the xor butterfly, then the four waves in order: a fixed order, the same on every run
#pragma unroll
    for (int q = 0; q < FM_REC; ++q) acc[q] = fm_wave_sum(acc[q]);
    if ((t & 63) == 0)
        for (int q = 0; q < FM_REC; ++q) red[t >> 6][q] = acc[q];
    __syncthreads();
    if (t < FM_REC) a.records[((long)n * a.n_tiles + tile) * FM_REC + t] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
}

// one wave per frame: lane l sums the records of tiles l, l + 64, ... in index order, the lanes meet in the butterfly; then
// out[0][n] = mse, out[1][n] = psnr, out[2][n] = ssim
__global__ __launch_bounds__(64) void frame_metrics_finish_kernel(const double* records, int n_tiles, int N, int h, int w, double range,
                                                                  double* out) {
    const int n = blockIdx.x, lane = threadIdx.x;
    double acc[FM_REC] = {0.0, 0.0, 0.0, 0.0};
    for (int tile = lane; tile < n_tiles; tile += 64)
        for (int q = 0; q < FM_REC; ++q) acc[q] += records[((long)n * n_tiles + tile) * FM_REC + q];
#pragma unroll
    for (int q = 0; q < FM_REC; ++q) acc[q] = fm_wave_sum(acc[q]);
    if (lane != 0) return;
    const double mse = acc[0] / (3.0 * (double)h * (double)w);
    const double count = (double)(h - 2 * FM_HALO) * (double)(w - 2 * FM_HALO);
    out[n] = mse;
    out[(long)N + n] = mse == 0.0 ? (double)INFINITY : 10.0 * log10((range * range) / mse);
    out[2 * (long)N + n] = ((acc[1] / count + acc[2] / count) + acc[3] / count) / 3.0;
}

long fm_tiles(int v) { return (v + FM_TILE - 1) / FM_TILE; }

// the largest element index the kernel can read stays inside [0, extent)
bool fm_source_ok(const orv_frames_t* f, int N, const char* who, const char* name) {
    if (!(f->kind == ORV_METRICS_SRC_F32 || f->kind == ORV_METRICS_SRC_U8)) {
        orv_set_error("%s: %s.kind = %d; supported: 0 (fp32), 1 (uint8, divided by 255)", who, name, f->kind);
        return false;
    }
    if (!(f->h >= 1 && f->w >= 1 && f->h <= 32768 && f->w <= 32768)) {
        orv_set_error("%s: %s is %d x %d; supported: 1 to 32768 per axis", who, name, f->h, f->w);
        return false;
    }
    long last = f->offset;
    bool ok = f->offset >= 0 && f->extent >= 1;
    const long span[4] = {N - 1, f->h - 1, f->w - 1, 2};
    for (int k = 0; k < 4 && ok; ++k) {
        ok = f->stride[k] >= 0 && (span[k] == 0 || f->stride[k] <= (f->extent - 1 - last) / span[k]);
        if (ok) last += span[k] * f->stride[k];
    }
    if (!ok || last >= f->extent) {
        orv_set_error("%s: bad strides: %s has offset %ld and element strides (n, y, x, c) = (%ld, %ld, %ld, %ld) over %d x %d x %d x 3 in a buffer of "
                      "%ld elements; supported: offset and strides >= 0 and every element inside the buffer",
                      who, name, f->offset, f->stride[0], f->stride[1], f->stride[2], f->stride[3], N, f->h, f->w, f->extent);
        return false;
    }
    return true;
}

}  // namespace

extern "C" long orv_frame_metrics_workspace(int N, int h, int w) {
    if (N < 0 || h < 1 || w < 1) return 0;
    return (long)N * fm_tiles(h) * fm_tiles(w) * FM_REC * (long)sizeof(double);
}

extern "C" int orv_frame_metrics(const orv_frames_t* pred, const orv_frames_t* gt, int N, int h, int w, double data_range, double* out,
                                 float* ssim_map, void* workspace, long workspace_bytes, void* stream) {
    const char* who = "orv_frame_metrics";
    ORV_REQUIRE(pred && gt, "%s: null pointer (pred / gt)", who);
    ORV_REQUIRE(N >= 0 && N <= 65535, "%s: N = %d frames; supported: 0 to 65535", who, N);
    ORV_REQUIRE(h >= 7 && w >= 7 && h <= 32768 && w <= 32768, "%s: the resized image is %d x %d; supported: 7 to 32768 per axis (one 7 x 7 window at least)", who, h, w);
    ORV_REQUIRE(data_range > 0.0 && data_range < 1e30, "%s: data_range = %g; supported: a positive finite range", who, data_range);
    if (N == 0) return ORV_OK;
    if (!fm_source_ok(pred, N, who, "pred") || !fm_source_ok(gt, N, who, "gt")) return ORV_EINVAL;
    ORV_REQUIRE(pred->data && gt->data && out && workspace, "%s: null pointer (pred.data / gt.data / out / workspace)", who);
    const long need = orv_frame_metrics_workspace(N, h, w);
    ORV_REQUIRE(workspace_bytes >= need, "%s: the workspace holds %ld bytes; orv_frame_metrics_workspace(%d, %d, %d) = %ld", who, workspace_bytes, N, h, w, need);
    ORV_REQUIRE(((uintptr_t)out & 7) == 0 && ((uintptr_t)workspace & 7) == 0 && ((uintptr_t)ssim_map & 3) == 0 &&
                    (pred->kind != ORV_METRICS_SRC_F32 || ((uintptr_t)pred->data & 3) == 0) && (gt->kind != ORV_METRICS_SRC_F32 || ((uintptr_t)gt->data & 3) == 0),
                "%s: out and workspace must be 8-byte, ssim_map and fp32 sources 4-byte aligned", who);
    FmArgs a;
    const orv_frames_t* in[2] = {pred, gt};
    for (int k = 0; k < 2; ++k) {
        FmSource& s = a.src[k];
        const long esize = in[k]->kind == ORV_METRICS_SRC_F32 ? 4 : 1;
        s.data = (const char*)in[k]->data + in[k]->offset * esize;
        s.sn = in[k]->stride[0], s.sy = in[k]->stride[1], s.sx = in[k]->stride[2], s.sc = in[k]->stride[3];
        s.kind = in[k]->kind, s.h = in[k]->h, s.w = in[k]->w;
    }
    a.records = (double*)workspace, a.ssim_map = ssim_map;
    a.N = N, a.h = h, a.w = w, a.tiles_x = (int)fm_tiles(w), a.n_tiles = (int)(fm_tiles(h) * fm_tiles(w));
    a.c1 = (float)((0.01 * data_range) * (0.01 * data_range)), a.c2 = (float)((0.03 * data_range) * (0.03 * data_range));
    hipLaunchKernelGGL(frame_metrics_kernel, dim3((unsigned)a.n_tiles, (unsigned)N), dim3(256), 0, (hipStream_t)stream, a);
    int rc = orv_check_launch(who);
    if (rc != ORV_OK) return rc;
    hipLaunchKernelGGL(frame_metrics_finish_kernel, dim3((unsigned)N), dim3(64), 0, (hipStream_t)stream, (const double*)workspace, a.n_tiles, N, h, w,
                       data_range, out);
    return orv_check_launch(who);
}
