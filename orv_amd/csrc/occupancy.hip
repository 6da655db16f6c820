// Occupancy labelling and sparse Gaussian scene preparation: the two pieces of ORV's conditioning chain between the point-cloud
// voxelization (voxelize.hip) and the Gaussian rasterizer (gs_render.hip).
//   * project_labels replaces project_3d_to_2d (orv/dataset/prepare_dataset.py:878-884) and the labelling block of get_occupancy
//     (:999-1008): about ten torch ops and several [N,4] temporaries per frame become one kernel, one thread per point.
//   * the scene kernels replace the front of get_render (:2069-2086 and :2148-2164), which per frame fills a 64 M-cell int64 grid, runs
//     torch.unique over it, builds a [64 M, 12] one-hot and gathers six dense attribute tensors by a boolean mask - to keep about 1e5
//     Gaussians.  Here nothing has the size of the grid: one int64 key per occupancy row, a stable sort of the keys (torch), one pass that
//     marks each cell's last row and ORs its label into a 64-bit class bitmap, a prefix sum (torch), one kernel that writes every attribute.
// Written from the arithmetic contract in DESIGN.md §14.  The only atomics are integer ORs (a flag, a bitmap): independent of order, so
// every output is bit-reproducible.
#include "common.hpp"

// The projection is defined on individually rounded fp32 products and sums and a correctly rounded fp32 division.  __fmul_rn / __fadd_rn of
// this toolchain are a plain product and sum inside a header compiled with contraction allowed, which the optimizer may still fuse after
// inlining; operators under this pragma carry no contract flag and cannot be fused.
#pragma clang fp contract(off)

namespace {

constexpr long OC_INVALID = 0x7fffffffffffffffL;     // key of a row outside the grid: sorts behind every cell
constexpr int OC_MAX_LABEL = 59;                     // len(colors60) - 1: labels are clamped to [0, 59], and 255 in the label image means 59
constexpr int OC_MAX_CHANNELS = 64;

__device__ __forceinline__ float oc_mul(float a, float b) { return a * b; }
__device__ __forceinline__ float oc_add(float a, float b) { return a + b; }
// ((x P[0] + y P[1]) + z P[2]) + P[3], every product and sum rounded to fp32 on its own
__device__ __forceinline__ float oc_row(const float* __restrict__ P, float x, float y, float z) {
    return oc_add(oc_add(oc_add(oc_mul(x, P[0]), oc_mul(y, P[1])), oc_mul(z, P[2])), P[3]);
}

// one thread per point: the pixel (u, v) = trunc(h_0 / h_2, h_1 / h_2) of the point under the 3 x 4 projection P, and the label under it
template <typename L>
__global__ __launch_bounds__(256) void oc_project_kernel(const float* __restrict__ points, int N, int C, const float* __restrict__ P,
                                                         const L* __restrict__ labels2d, int H, int W, long* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const float* p = points + (long)i * C;
    const float x = p[0], y = p[1], z = p[2];
    const float h0 = oc_row(P, x, y, z), h1 = oc_row(P + 4, x, y, z), h2 = oc_row(P + 8, x, y, z);
    const float u = h0 / h2, v = h1 / h2;
    long label = 0;
    // trunc(u) in [0, W) is u in (-1, W): a value in (-1, 0) truncates to 0.  NaN and +-inf compare false and stay outside.
    if (u > -1.0f && u < (float)W && v > -1.0f && v < (float)H) {
        label = (long)labels2d[(long)(int)v * W + (int)u];
        if (label == 255 || label == -1) label = OC_MAX_LABEL;
    }
    out[i] = label;
}

// one thread per occupancy row (x, y, z, label): the dense linear index (x Y + y) Z + z; a row outside the grid raises the flag
__global__ __launch_bounds__(256) void oc_keys_kernel(const int* __restrict__ occ, int M, int X, int Y, int Z, long* __restrict__ keys,
                                                      long* __restrict__ state) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    const int4 r = *(const int4*)(occ + 4 * (long)i);
    const bool ok = (unsigned)r.x < (unsigned)X && (unsigned)r.y < (unsigned)Y && (unsigned)r.z < (unsigned)Z;
    keys[i] = ok ? ((long)r.x * Y + r.y) * Z + r.z : OC_INVALID;
    if (!ok) atomicOr((unsigned long long*)(state + 1), 1ULL);
}

__device__ __forceinline__ int oc_label(const int* __restrict__ occ, unsigned long row) {
    const int l = occ[4 * row + 3];
    return l < 0 ? 0 : (l > OC_MAX_LABEL ? OC_MAX_LABEL : l);
}

// one thread per sorted entry: last[j] = 1 when the entry closes its cell's segment (the sort is stable, so that is the cell's last row,
// the one whose label the dense scatter keeps); the clamped labels of those rows are ORed into state[0], one atomic per wave
__global__ __launch_bounds__(256) void oc_mark_kernel(const long* __restrict__ keys, const long* __restrict__ order,
                                                      const int* __restrict__ occ, int M, int* __restrict__ last, long* __restrict__ state) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    unsigned long long bits = 0;
    if (j < M) {
        const long k = keys[j];
        const unsigned long row = (unsigned long)order[j];
        const bool closes = k != OC_INVALID && row < (unsigned long)M && (j == M - 1 || keys[j + 1] != k);
        last[j] = closes ? 1 : 0;
        if (closes) bits = 1ULL << oc_label(occ, row);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) bits |= __shfl_xor(bits, off, 64);
    if ((threadIdx.x & 63) == 0 && bits) atomicOr((unsigned long long*)state, bits);
}

struct OcWriteArgs {
    const long* order;
    const int *occ, *last, *csum;
    const float *ax, *ay, *az, *zscale;
    float *xyz, *rgb, *feat, *rot, *scale, *opacity;
    unsigned long long classes;                       // the class bitmap, with bit 0 set when the grid has an empty cell
    int M, n, X, Y, Z, F;
};

// one thread per sorted entry: the entry that closes cell number g = csum[j] - 1 (cells in ascending order of the dense index) writes every
// attribute of Gaussian g; the one-hot's channel is the label's rank among the classes present: the popcount of the bitmap below the label
__global__ __launch_bounds__(256) void oc_write_kernel(const OcWriteArgs a) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= a.M || !a.last[j]) return;
    const int g = a.csum[j] - 1;
    const unsigned long row = (unsigned long)a.order[j];
    if (g < 0 || g >= a.n || row >= (unsigned long)a.M) return;
    const int4 r = *(const int4*)(a.occ + 4 * row);              // the row holds the cell's coordinates: no need to take the key apart
    const int x = r.x, y = r.y, z = r.z;
    if ((unsigned)x >= (unsigned)a.X || (unsigned)y >= (unsigned)a.Y || (unsigned)z >= (unsigned)a.Z) return;
    const int label = r.w < 0 ? 0 : (r.w > OC_MAX_LABEL ? OC_MAX_LABEL : r.w);
    const int rank = __popcll(a.classes & ((1ULL << label) - 1ULL));
    const long g3 = 3 * (long)g;
    a.xyz[g3] = a.ax[x], a.xyz[g3 + 1] = a.ay[y], a.xyz[g3 + 2] = a.az[z];
    a.rgb[g3] = 0.0f, a.rgb[g3 + 1] = 0.0f, a.rgb[g3 + 2] = 0.0f;
    const float s = a.zscale[z];
    a.scale[g3] = s, a.scale[g3 + 1] = s, a.scale[g3 + 2] = s;
    *(float4*)(a.rot + 4 * (long)g) = make_float4(1.0f, 0.0f, 0.0f, 0.0f);
    a.opacity[g] = 1.0f;
    float* f = a.feat + (long)g * a.F;
    for (int c = 0; c < a.F; ++c) f[c] = c == rank ? 1.0f : 0.0f;
}

}  // namespace

extern "C" int orv_occ_project_labels(const float* points, int N, int C, const float* P, const void* labels2d, int label_bytes, int H, int W,
                                      long* labels3d, void* stream) {
    ORV_REQUIRE(N >= 0, "orv_occ_project_labels: N must not be negative (got %d)", N);
    ORV_REQUIRE(C >= 3, "orv_occ_project_labels: C = %d features per point; supported: C >= 3 (x, y, z first)", C);
    ORV_REQUIRE(H >= 1 && W >= 1 && (long)H * W < 2147483648L, "orv_occ_project_labels: the label image is %d x %d; supported: H, W >= 1 and H W < 2^31", H, W);
    ORV_REQUIRE(label_bytes == 1 || label_bytes == 4, "orv_occ_project_labels: label_bytes = %d; supported: 1 (uint8) or 4 (int32)", label_bytes);
    if (N == 0) return ORV_OK;
    ORV_REQUIRE(points && P && labels2d && labels3d, "orv_occ_project_labels: null pointer (points / P / labels2d / labels3d)");
    ORV_REQUIRE(orv_aligned(points, 4) && orv_aligned(P, 4) && orv_aligned(labels2d, (uintptr_t)label_bytes) && orv_aligned(labels3d, 8),
                "orv_occ_project_labels: points and P must be 4-byte, labels2d element and labels3d 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (label_bytes == 1)
        hipLaunchKernelGGL(oc_project_kernel<unsigned char>, dim3(orv_blocks(N, 256)), dim3(256), 0, s, points, N, C, P, (const unsigned char*)labels2d, H, W, labels3d);
    else
        hipLaunchKernelGGL(oc_project_kernel<int>, dim3(orv_blocks(N, 256)), dim3(256), 0, s, points, N, C, P, (const int*)labels2d, H, W, labels3d);
    return orv_check_launch("orv_occ_project_labels");
}

static int oc_check_grid(const char* who, int X, int Y, int Z) {
    ORV_REQUIRE(X >= 1 && Y >= 1 && Z >= 1 && X <= 65535 && Y <= 65535 && Z <= 65535,
                "%s: the grid is %d x %d x %d cells; supported: 1 to 65535 cells on every axis", who, X, Y, Z);
    return ORV_OK;
}

extern "C" int orv_occ_cell_keys(const int* occ, int M, int X, int Y, int Z, long* keys, long* state, void* stream) {
    ORV_REQUIRE(M >= 0, "orv_occ_cell_keys: M must not be negative (got %d)", M);
    if (int e = oc_check_grid("orv_occ_cell_keys", X, Y, Z)) return e;
    if (M == 0) return ORV_OK;
    ORV_REQUIRE(occ && keys && state, "orv_occ_cell_keys: null pointer (occ / keys / state)");
    ORV_REQUIRE(orv_aligned(occ, 16) && orv_aligned(keys, 8) && orv_aligned(state, 8), "orv_occ_cell_keys: occ must be 16-byte, keys and state 8-byte aligned");
    hipLaunchKernelGGL(oc_keys_kernel, dim3(orv_blocks(M, 256)), dim3(256), 0, (hipStream_t)stream, occ, M, X, Y, Z, keys, state);
    return orv_check_launch("orv_occ_cell_keys");
}

extern "C" int orv_occ_mark_cells(const long* sorted_keys, const long* order, const int* occ, int M, int* last, long* state, void* stream) {
    ORV_REQUIRE(M >= 0, "orv_occ_mark_cells: M must not be negative (got %d)", M);
    if (M == 0) return ORV_OK;
    ORV_REQUIRE(sorted_keys && order && occ && last && state, "orv_occ_mark_cells: null pointer");
    ORV_REQUIRE(orv_aligned(sorted_keys, 8) && orv_aligned(order, 8) && orv_aligned(state, 8) && orv_aligned(occ, 4) && orv_aligned(last, 4),
                "orv_occ_mark_cells: sorted_keys, order and state must be 8-byte, occ and last 4-byte aligned");
    hipLaunchKernelGGL(oc_mark_kernel, dim3(orv_blocks(M, 256)), dim3(256), 0, (hipStream_t)stream, sorted_keys, order, occ, M, last, state);
    return orv_check_launch("orv_occ_mark_cells");
}

extern "C" int orv_occ_write_gaussians(const long* order, const int* occ, const int* last, const int* csum, int M,
                                       int n, int X, int Y, int Z, const float* ax, const float* ay, const float* az, const float* zscale,
                                       unsigned long classes, int F, float* xyz, float* rgb, float* feat, float* rot, float* scale,
                                       float* opacity, void* stream) {
    ORV_REQUIRE(M >= 0, "orv_occ_write_gaussians: M must not be negative (got %d)", M);
    ORV_REQUIRE(n >= 0 && n <= M, "orv_occ_write_gaussians: n = %d Gaussians must be in [0, M = %d]", n, M);
    if (int e = oc_check_grid("orv_occ_write_gaussians", X, Y, Z)) return e;
    ORV_REQUIRE(F >= 1 && F <= OC_MAX_CHANNELS, "orv_occ_write_gaussians: F = %d feature channels; supported: 1 to %d", F, OC_MAX_CHANNELS);
    int ranks = 0;
    for (unsigned long b = classes; b; b &= b - 1) ++ranks;
    ORV_REQUIRE((classes >> (OC_MAX_LABEL + 1)) == 0 && ranks <= F,
                "orv_occ_write_gaussians: the class bitmap holds %d classes (labels 0 to %d only) for F = %d channels", ranks, OC_MAX_LABEL, F);
    if (M == 0 || n == 0) return ORV_OK;
    ORV_REQUIRE(order && occ && last && csum, "orv_occ_write_gaussians: null pointer (an input array)");
    ORV_REQUIRE(ax && ay && az && zscale, "orv_occ_write_gaussians: null pointer (a table)");
    ORV_REQUIRE(xyz && rgb && feat && rot && scale && opacity, "orv_occ_write_gaussians: null pointer (an output buffer)");
    ORV_REQUIRE(orv_aligned(order, 8) && orv_aligned(occ, 16) && orv_aligned(rot, 16),
                "orv_occ_write_gaussians: order must be 8-byte, occ and rot 16-byte aligned");
    OcWriteArgs a;
    a.order = order, a.occ = occ, a.last = last, a.csum = csum;
    a.ax = ax, a.ay = ay, a.az = az, a.zscale = zscale;
    a.xyz = xyz, a.rgb = rgb, a.feat = feat, a.rot = rot, a.scale = scale, a.opacity = opacity;
    a.classes = classes, a.M = M, a.n = n, a.X = X, a.Y = Y, a.Z = Z, a.F = F;
    hipLaunchKernelGGL(oc_write_kernel, dim3(orv_blocks(M, 256)), dim3(256), 0, (hipStream_t)stream, a);
    return orv_check_launch("orv_occ_write_gaussians");
}
