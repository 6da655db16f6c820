// Point-cloud voxelization behind ORV's occupancy preparation (the reference voxelizes every frame's point cloud through the CUDA extension
// orv/ops/voxelize, called by points_to_voxels, orv/dataset/prepare_dataset.py:137-198, from get_occupancy, :887-1039).
// Written from the arithmetic contract in DESIGN.md §13, whose definition is the sequential walk of orv/ops/voxelize/voxelization_cpu.cpp:71-102:
// one int64 voxel key per point, a stable sort of the keys (torch), segments of equal keys found by binary search in the sorted list, the
// voxels numbered in order of first appearance by a prefix sum over "this point opens a voxel" flags (torch), then either the scatter of the
// kept points into voxels[M, max_points, C] or the fused semantic vote that never builds that buffer.  No thread walks all points and no
// result depends on the order of an atomic: the output is bit-reproducible and equal to the sequential definition.
#include "common.hpp"

// the cell of a point is defined on an individually rounded fp32 subtraction and a correctly rounded fp32 division
#pragma clang fp contract(off)

namespace {

constexpr long VX_INVALID = 0x7fffffffffffffffL;     // key of a point outside the grid: sorts behind every cell
constexpr int VX_LABELS = 256;                       // stored labels 1..255 (label + 1); 0 is padding

struct VxGrid {
    float vs[3], lo[3];
    int g[3];                                        // cells along x, y, z
};

// (int) floorf((p - lo) / vs) when that is a cell of the axis, else -1 (NaN and +-inf compare false and fall out here)
__device__ __forceinline__ int vx_cell(float p, float lo, float vs, int g) {
    const float f = floorf((p - lo) / vs);
    if (!(f >= 0.0f && f < 2147483648.0f)) return -1;
    const int c = (int)f;
    return c < g ? c : -1;
}

// one thread per point: coors [N,3] (z, y, x) or (-1, -1, -1), and the linear cell key
__global__ __launch_bounds__(256) void vx_coors_kernel(const float* __restrict__ points, int N, int C, const VxGrid gr,
                                                       int* __restrict__ coors, long* __restrict__ keys) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const float* p = points + (long)i * C;
    int cx = vx_cell(p[0], gr.lo[0], gr.vs[0], gr.g[0]);
    int cy = vx_cell(p[1], gr.lo[1], gr.vs[1], gr.g[1]);
    int cz = vx_cell(p[2], gr.lo[2], gr.vs[2], gr.g[2]);
    const bool ok = (cx | cy | cz) >= 0;
    if (!ok) cx = cy = cz = -1;
    coors[3 * (long)i] = cz, coors[3 * (long)i + 1] = cy, coors[3 * (long)i + 2] = cx;
    if (keys) keys[i] = ok ? ((long)cz * gr.g[1] + cy) * gr.g[0] + cx : VX_INVALID;
}

// first position in the sorted keys [0, n) whose key is >= k (upper = false) or > k (upper = true)
__device__ __forceinline__ int vx_bound(const long* __restrict__ keys, int n, long k, bool upper) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        const long v = keys[mid];
        if (upper ? v <= k : v < k) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// one thread per sorted entry: the position of its segment's head; the head also writes the segment's length and flags its point (the
// voxel's first point, because the sort is stable) in first[N].  Entries of invalid points get start = -1.
__global__ __launch_bounds__(256) void vx_segments_kernel(const long* __restrict__ keys, const long* __restrict__ order, int N,
                                                          int* __restrict__ start, int* __restrict__ seglen, int* __restrict__ first) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= N) return;
    const long k = keys[j];
    if (k == VX_INVALID) {
        start[j] = -1, seglen[j] = 0;
        return;
    }
    const bool head = j == 0 || keys[j - 1] != k;
    const int h = head ? j : vx_bound(keys, j, k, false);
    start[j] = h;
    seglen[j] = 0;
    if (head) {
        seglen[j] = vx_bound(keys + j, N - j, k, true);
        const unsigned long p = (unsigned long)order[j];
        if (p < (unsigned long)N) first[p] = 1;
    }
}

struct VxScatterArgs {
    const float* points;
    const int *pt_coors, *start, *seglen, *csum;
    const long* order;
    float* voxels;
    int *coors, *num;
    int N, C, max_points, M;
};

// one thread per sorted entry: a point of a kept voxel (number < M) below the per-voxel cap copies its C features into its slot; the head
// also writes the voxel's coordinates and min(length, max_points)
__global__ __launch_bounds__(256) void vx_scatter_kernel(const VxScatterArgs a) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= a.N) return;
    const int h = a.start[j];
    if (h < 0 || h > j) return;
    const int rank = j - h;
    if (rank >= a.max_points) return;
    const unsigned long p0 = (unsigned long)a.order[h], p = (unsigned long)a.order[j];
    if (p0 >= (unsigned long)a.N || p >= (unsigned long)a.N) return;
    const int v = a.csum[p0] - 1;
    if (v < 0 || v >= a.M) return;
    const float* src = a.points + (long)p * a.C;
    float* dst = a.voxels + ((long)v * a.max_points + rank) * a.C;
    for (int k = 0; k < a.C; ++k) dst[k] = src[k];
    if (rank == 0) {
        const int len = a.seglen[h];
        a.coors[3 * (long)v] = a.pt_coors[3 * p0], a.coors[3 * (long)v + 1] = a.pt_coors[3 * p0 + 1], a.coors[3 * (long)v + 2] = a.pt_coors[3 * p0 + 2];
        a.num[v] = len < a.max_points ? len : a.max_points;
    }
}

// one thread per sorted entry: the head of kept voxel v records its sorted position in head_of[v]
__global__ __launch_bounds__(256) void vx_heads_kernel(const long* __restrict__ order, const int* __restrict__ start,
                                                       const int* __restrict__ csum, int N, int M, int* __restrict__ head_of) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= N || start[j] != j) return;
    const unsigned long p0 = (unsigned long)order[j];
    if (p0 >= (unsigned long)N) return;
    const int v = csum[p0] - 1;
    if (v >= 0 && v < M) head_of[v] = j;
}

struct VxVoteArgs {
    const float* points;
    const int *pt_coors, *seglen, *head_of;
    const long* order;
    int* out;
    int N, C, max_points, M;
};

// One wave per kept voxel: the stored labels (last feature, label + 1) of the voxel's first min(length, max_points) points are counted in
// a 256-bin LDS histogram of the wave (integer counts: the order of the adds does not matter), every lane takes four bins, and a butterfly
// picks the largest count, a tie going to the smaller label.  out[v] = (x, y, z, label); label = -1 when no point carried a stored label in
// 1..255 (outside the contract).
__global__ __launch_bounds__(256) void vx_vote_kernel(const VxVoteArgs a) {
    __shared__ int s_hist[4][VX_LABELS];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int v = blockIdx.x * 4 + w;                // wave-uniform; a wave past the last voxel counts nothing and writes nothing
    int* hist = s_hist[w];
#pragma unroll
    for (int k = 0; k < VX_LABELS / 64; ++k) hist[lane + 64 * k] = 0;
    const int h = v < a.M ? a.head_of[v] : -1;
    int cnt = 0;
    unsigned long p0 = 0;
    if (h >= 0 && h < a.N) {
        cnt = a.seglen[h];
        cnt = cnt < a.max_points ? cnt : a.max_points;
        cnt = cnt < a.N - h ? cnt : a.N - h;
        p0 = (unsigned long)a.order[h];
    }
    __syncthreads();
    for (int e = lane; e < cnt; e += 64) {
        const unsigned long p = (unsigned long)a.order[h + e];
        if (p < (unsigned long)a.N) {
            const float s = a.points[(long)p * a.C + (a.C - 1)];
            if (s >= 1.0f && s < (float)VX_LABELS) atomicAdd(&hist[(int)s], 1);
        }
    }
    __syncthreads();
    int best_c = 0, best_l = 0;
#pragma unroll
    for (int k = 0; k < VX_LABELS / 64; ++k) {
        const int l = lane * (VX_LABELS / 64) + k, c = hist[l];     // ascending labels within a lane: '>' keeps the smaller on a tie
        if (l > 0 && c > best_c) best_c = c, best_l = l;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int oc = __shfl_xor(best_c, off), ol = __shfl_xor(best_l, off);
        if (oc > best_c || (oc == best_c && oc > 0 && ol < best_l)) best_c = oc, best_l = ol;
    }
    if (lane == 0 && v < a.M) {
        int x = -1, y = -1, z = -1;
        if (p0 < (unsigned long)a.N && cnt > 0) z = a.pt_coors[3 * p0], y = a.pt_coors[3 * p0 + 1], x = a.pt_coors[3 * p0 + 2];
        *(int4*)(a.out + 4 * (long)v) = make_int4(x, y, z, best_l - 1);
    }
}

// grid size per axis by the reference's rule, round((hi - lo) / vs) in fp32 (voxelization_cpu.cpp:118-121); false when an axis has no cell
inline bool vx_grid(const float* vs, const float* range, VxGrid* gr) {
    for (int a = 0; a < 3; ++a) {
        const float span = range[3 + a] - range[a];
        const float q = span / vs[a];
        const float r = roundf(q);
        if (!(vs[a] > 0.0f) || !(r >= 1.0f && r < 2147483648.0f)) return false;
        gr->vs[a] = vs[a], gr->lo[a] = range[a], gr->g[a] = (int)r;
    }
    return true;
}

}  // namespace

extern "C" int orv_voxel_grid_size(float vx, float vy, float vz, float x0, float y0, float z0, float x1, float y1, float z1, int* grid) {
    ORV_REQUIRE(grid, "orv_voxel_grid_size: null pointer (grid)");
    const float vs[3] = {vx, vy, vz}, range[6] = {x0, y0, z0, x1, y1, z1};
    ORV_REQUIRE(vx > 0.0f && vy > 0.0f && vz > 0.0f, "orv_voxel_grid_size: the voxel size must be positive (got %g, %g, %g)", vx, vy, vz);
    VxGrid gr;
    ORV_REQUIRE(vx_grid(vs, range, &gr), "orv_voxel_grid_size: the grid round((max - min) / voxel_size) must have 1 to 2^31 - 1 cells on every axis");
    grid[0] = gr.g[0], grid[1] = gr.g[1], grid[2] = gr.g[2];
    return ORV_OK;
}

extern "C" int orv_voxel_coors(const float* points, int N, int C, float vx, float vy, float vz, float x0, float y0, float z0, float x1,
                               float y1, float z1, int* coors, long* keys, void* stream) {
    ORV_REQUIRE(N >= 0, "orv_voxel_coors: N must not be negative (got %d)", N);
    ORV_REQUIRE(C >= 3, "orv_voxel_coors: C = %d features per point; supported: C >= 3 (x, y, z first)", C);
    const float vs[3] = {vx, vy, vz}, range[6] = {x0, y0, z0, x1, y1, z1};
    ORV_REQUIRE(vx > 0.0f && vy > 0.0f && vz > 0.0f, "orv_voxel_coors: the voxel size must be positive (got %g, %g, %g)", vx, vy, vz);
    VxGrid gr;
    ORV_REQUIRE(vx_grid(vs, range, &gr), "orv_voxel_coors: the grid round((max - min) / voxel_size) must have 1 to 2^31 - 1 cells on every axis");
    ORV_REQUIRE(!keys || (double)gr.g[0] * gr.g[1] * gr.g[2] < 4.0e18, "orv_voxel_coors: %d x %d x %d cells do not fit a 63-bit key", gr.g[0], gr.g[1], gr.g[2]);
    if (N == 0) return ORV_OK;
    ORV_REQUIRE(points && coors, "orv_voxel_coors: null pointer (points / coors)");
    ORV_REQUIRE(orv_aligned(keys, 8), "orv_voxel_coors: keys must be 8-byte aligned");
    hipLaunchKernelGGL(vx_coors_kernel, dim3((unsigned)(((long)N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, points, N, C, gr, coors, keys);
    return orv_check_launch("orv_voxel_coors");
}

extern "C" int orv_voxel_segments(const long* sorted_keys, const long* order, int N, int* start, int* seglen, int* first, void* stream) {
    ORV_REQUIRE(N >= 0, "orv_voxel_segments: N must not be negative (got %d)", N);
    if (N == 0) return ORV_OK;
    ORV_REQUIRE(sorted_keys && order && start && seglen && first, "orv_voxel_segments: null pointer");
    ORV_REQUIRE(orv_aligned(sorted_keys, 8) && orv_aligned(order, 8), "orv_voxel_segments: sorted_keys and order must be 8-byte aligned");
    hipLaunchKernelGGL(vx_segments_kernel, dim3((unsigned)(((long)N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, sorted_keys, order, N, start,
                       seglen, first);
    return orv_check_launch("orv_voxel_segments");
}

extern "C" int orv_voxel_scatter(const float* points, const int* point_coors, const long* order, const int* start, const int* seglen,
                                 const int* csum, int N, int C, int max_points, int M, float* voxels, int* coors,
                                 int* num_points_per_voxel, void* stream) {
    ORV_REQUIRE(N >= 0, "orv_voxel_scatter: N must not be negative (got %d)", N);
    ORV_REQUIRE(C >= 3, "orv_voxel_scatter: C = %d features per point; supported: C >= 3 (x, y, z first)", C);
    ORV_REQUIRE(max_points > 0, "orv_voxel_scatter: max_points must be positive (got %d)", max_points);
    ORV_REQUIRE(M >= 0 && M <= N, "orv_voxel_scatter: M = %d voxels must be in [0, N = %d]", M, N);
    if (N == 0 || M == 0) return ORV_OK;
    ORV_REQUIRE(points && point_coors && order && start && seglen && csum, "orv_voxel_scatter: null pointer (an input array)");
    ORV_REQUIRE(voxels && coors && num_points_per_voxel, "orv_voxel_scatter: null pointer (an output buffer)");
    ORV_REQUIRE(orv_aligned(order, 8), "orv_voxel_scatter: order must be 8-byte aligned");
    VxScatterArgs a;
    a.points = points, a.pt_coors = point_coors, a.order = order, a.start = start, a.seglen = seglen, a.csum = csum;
    a.voxels = voxels, a.coors = coors, a.num = num_points_per_voxel, a.N = N, a.C = C, a.max_points = max_points, a.M = M;
    hipLaunchKernelGGL(vx_scatter_kernel, dim3((unsigned)(((long)N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    return orv_check_launch("orv_voxel_scatter");
}

extern "C" int orv_voxel_vote(const float* points, const int* point_coors, const long* order, const int* start, const int* seglen,
                              const int* csum, int N, int C, int max_points, int M, int* head_of, int* out, void* stream) {
    ORV_REQUIRE(N >= 0, "orv_voxel_vote: N must not be negative (got %d)", N);
    ORV_REQUIRE(C >= 4, "orv_voxel_vote: C = %d features per point; supported: C >= 4 (x, y, z first, the stored label last)", C);
    ORV_REQUIRE(max_points > 0, "orv_voxel_vote: max_points must be positive (got %d)", max_points);
    ORV_REQUIRE(M >= 0 && M <= N, "orv_voxel_vote: M = %d voxels must be in [0, N = %d]", M, N);
    if (N == 0 || M == 0) return ORV_OK;
    ORV_REQUIRE(points && point_coors && order && start && seglen && csum, "orv_voxel_vote: null pointer (an input array)");
    ORV_REQUIRE(head_of && out, "orv_voxel_vote: null pointer (head_of / out)");
    ORV_REQUIRE(orv_aligned(order, 8) && orv_aligned(out, 16), "orv_voxel_vote: order must be 8-byte and out 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(vx_heads_kernel, dim3((unsigned)(((long)N + 255) / 256)), dim3(256), 0, s, order, start, csum, N, M, head_of);
    VxVoteArgs a;
    a.points = points, a.pt_coors = point_coors, a.order = order, a.seglen = seglen, a.head_of = head_of, a.out = out;
    a.N = N, a.C = C, a.max_points = max_points, a.M = M;
    hipLaunchKernelGGL(vx_vote_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, s, a);
    return orv_check_launch("orv_voxel_vote");
}
