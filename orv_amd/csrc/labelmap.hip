// Label-map compositing: a video segmenter's per-object masks to the 2-D label image and its colour preview, the last non-network step of
// ORV's label preparation (_postprocess_labels, orv/dataset/prepare_dataset.py:1377-1486).
//   * mask_stats replaces sv.mask_to_xyxy and detections.area (:1406-1420) and, for fp32 logits, the threshold of :1275-1279: the count
//     of set pixels and their inclusive bounding box per (frame, mask) plane.  Row-wise, one record per row band, a fixed-order second
//     pass: no atomics at all.
//   * compose replaces the 2 n boolean-index stores per frame of :1412-1444: one lane owns 16 consecutive pixels, keeps their label bytes
//     in four registers and walks the paint order once; colours are expanded at the end from a 256-entry table in LDS.
// Written from the contract in DESIGN.md §18.  Every value is an integer: outputs are bit-reproducible.
#include <vector>

#include "common.hpp"

namespace {

constexpr int LM_MAX_DIM = 65535;                    // H and W below 65536: x and y fit 16 bits, H W fits 32
constexpr int LM_MAX_MASKS = 1 << 24;                // a paint step packs the mask number in 24 bits next to its label byte
constexpr long LM_MAX_STRIDE = 1L << 40;
constexpr int LM_TABLE = 256;                        // id -> colour triple
constexpr int LM_GRID_CAP = 2048;                    // memory-bound: about 8 workgroups per CU, the rest by grid stride

// x > threshold in IEEE terms on the bits alone, so the device's denormal mode has no say: key() maps a float's bits to an int32 that
// orders like the float (-0 and +0 both 0); a NaN on either side compares false.  tkey = key(threshold), or INT_MAX for a NaN threshold.
__host__ __device__ __forceinline__ int lm_key(unsigned b) { return (b & 0x80000000u) ? -(int)(b & 0x7fffffffu) : (int)b; }
__device__ __forceinline__ bool lm_set_f32(unsigned b, int tkey) { return (b & 0x7fffffffu) <= 0x7f800000u && lm_key(b) > tkey; }
// 4 mask bytes -> 0xFF where the byte is nonzero, 0x00 elsewhere
__device__ __forceinline__ unsigned lm_sel_bytes4(unsigned w) {
    const unsigned t = ((w & 0x7f7f7f7fu) + 0x7f7f7f7fu) | w;      // bit 7 of every byte: byte != 0
    return ((t >> 7) & 0x01010101u) * 0xffu;
}
// 4 logits -> the same byte selects
__device__ __forceinline__ unsigned lm_sel_f32x4(uint4 v, int tkey) {
    return (lm_set_f32(v.x, tkey) ? 0x000000ffu : 0u) | (lm_set_f32(v.y, tkey) ? 0x0000ff00u : 0u) |
           (lm_set_f32(v.z, tkey) ? 0x00ff0000u : 0u) | (lm_set_f32(v.w, tkey) ? 0xff000000u : 0u);
}
// byte selects of 4 pixels -> 4 bits, pixel 0 in bit 0
__device__ __forceinline__ unsigned lm_bits4(unsigned sel) { return (((sel & 0x01010101u) * 0x01020408u) >> 24) & 0xfu; }

template <int MB>
__device__ __forceinline__ bool lm_set_at(const unsigned char* p, long i, int tkey) {
    if (MB == 1) return p[i] != 0;
    return lm_set_f32(((const unsigned*)p)[i], tkey);
}

// ---- stats ----
struct LmStat { unsigned area; int xmin, ymin, xmax, ymax; };

__device__ __forceinline__ void lm_stat_add(LmStat& s, unsigned bits, int x0, int y) {        // bits: pixel x0 + i in bit i
    if (!bits) return;
    s.area += __popc(bits);
    s.xmin = min(s.xmin, x0 + __ffs(bits) - 1), s.xmax = max(s.xmax, x0 + 31 - __clz(bits));
    s.ymin = min(s.ymin, y), s.ymax = max(s.ymax, y);
}

// workgroup b works on band b % bands of plane b / bands: rows [band H / bands, (band + 1) H / bands), a row per wave at a time.  A row is
// a byte-wise head up to the first 16-byte boundary, aligned 16-byte chunks a lane each, and a byte-wise tail: nothing outside the row is read.
template <int MB>
__global__ __launch_bounds__(256) void lm_stats_kernel(const unsigned char* __restrict__ masks, int n, int H, int W, long stride_f, long stride_n,
                                                       int tkey, int bands, int* __restrict__ ws) {
    constexpr int PPC = 16 / MB;                                         // pixels per 16-byte chunk
    const long plane = blockIdx.x / bands;
    const int band = blockIdx.x - plane * bands;
    const long f = plane / n, j = plane - f * n;
    const unsigned char* base = masks + (f * stride_f + j * stride_n) * MB;
    const int r0 = (int)((long)band * H / bands), r1 = (int)((long)(band + 1) * H / bands);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    LmStat s = {0u, 0x7fffffff, 0x7fffffff, -1, -1};
    for (int y = r0 + wave; y < r1; y += 4) {
        const unsigned char* row = base + (long)y * W * MB;
        const int head = min(W, (int)((16 - ((uintptr_t)row & 15)) & 15) / MB);
        const int chunks = (W - head) / PPC, tail0 = head + chunks * PPC;
        for (int c = lane; c < chunks; c += 64) {
            const uint4 v = *(const uint4*)(row + ((long)head + (long)c * PPC) * MB);
            unsigned bits;
            if (MB == 1)
                bits = lm_bits4(lm_sel_bytes4(v.x)) | lm_bits4(lm_sel_bytes4(v.y)) << 4 | lm_bits4(lm_sel_bytes4(v.z)) << 8 | lm_bits4(lm_sel_bytes4(v.w)) << 12;
            else
                bits = lm_bits4(lm_sel_f32x4(v, tkey));
            lm_stat_add(s, bits, head + c * PPC, y);
        }
        for (int i = lane; i < head + W - tail0; i += 64) {               // at most 15 + 15 pixels
            const int x = i < head ? i : tail0 + (i - head);
            lm_stat_add(s, lm_set_at<MB>(row, x, tkey) ? 1u : 0u, x, y);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s.area += __shfl_xor(s.area, o, 64);
        s.xmin = min(s.xmin, __shfl_xor(s.xmin, o, 64)), s.ymin = min(s.ymin, __shfl_xor(s.ymin, o, 64));
        s.xmax = max(s.xmax, __shfl_xor(s.xmax, o, 64)), s.ymax = max(s.ymax, __shfl_xor(s.ymax, o, 64));
    }
    __shared__ LmStat part[4];
    if (lane == 0) part[wave] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) {
            s.area += part[w].area;
            s.xmin = min(s.xmin, part[w].xmin), s.ymin = min(s.ymin, part[w].ymin);
            s.xmax = max(s.xmax, part[w].xmax), s.ymax = max(s.ymax, part[w].ymax);
        }
        int* rec = ws + 5 * (long)blockIdx.x;
        rec[0] = (int)s.area, rec[1] = s.xmin, rec[2] = s.ymin, rec[3] = s.xmax, rec[4] = s.ymax;
    }
}

// one thread per plane: its bands in order, widened to int64; an empty mask gives all zeros (sv.mask_to_xyxy)
__global__ __launch_bounds__(256) void lm_stats_final_kernel(const int* __restrict__ ws, long planes, int bands, long* __restrict__ area,
                                                             long* __restrict__ xyxy) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= planes) return;
    long a = 0;
    int xmin = 0x7fffffff, ymin = 0x7fffffff, xmax = -1, ymax = -1;
    for (int b = 0; b < bands; ++b) {
        const int* rec = ws + 5 * (p * bands + b);
        a += (long)(unsigned)rec[0];
        xmin = min(xmin, rec[1]), ymin = min(ymin, rec[2]), xmax = max(xmax, rec[3]), ymax = max(ymax, rec[4]);
    }
    area[p] = a;
    long* box = xyxy + 4 * p;
    box[0] = a ? xmin : 0, box[1] = a ? ymin : 0, box[2] = a ? xmax : 0, box[3] = a ? ymax : 0;
}

// ---- compose ----
struct LmComposeArgs {
    const unsigned char* masks;
    const unsigned* steps;                            // [m] paint steps (label << 24 | mask number), then the 256-entry colour table
    unsigned char *index, *color;
    long stride_f, stride_n, HW, groups, total;       // groups = ceil(HW / 16) per frame, total = F groups
    int m, tkey;
};

// one lane per group of 16 consecutive pixels of a frame's flat plane.  Its 16 label bytes sit in lab[4] and the painted selects in
// painted[4] (a byte of 0xFF per painted pixel: the 16-bit painted mask, kept unpacked so that a step costs one OR per 4 pixels, not a
// pack); a step loads the group's 16 mask bytes (or 16 logits by four loads), turns them into byte selects and merges the step's label by
// a bitfield insert per 4 pixels.  A plane whose group is not 16-byte aligned, and the last partial group, go element by element.
template <int MB>
__global__ __launch_bounds__(256) void lm_compose_kernel(const LmComposeArgs a) {
    __shared__ unsigned table[LM_TABLE];
    table[threadIdx.x] = a.steps[a.m + threadIdx.x];
    __syncthreads();
    for (long item = (long)blockIdx.x * 256 + threadIdx.x; item < a.total; item += (long)gridDim.x * 256) {
        const long f = item / a.groups, p0 = (item - f * a.groups) * 16;
        const int cnt = (int)min(16L, a.HW - p0);
        const unsigned char* src = a.masks + (f * a.stride_f + p0) * MB;
        unsigned lab[4] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu}, painted[4] = {0u, 0u, 0u, 0u};
        for (int k = 0; k < a.m; ++k) {
            const unsigned step = a.steps[k];
            const unsigned char* p = src + (long)(step & 0xffffffu) * a.stride_n * MB;
            unsigned sel[4];
            if (cnt == 16 && ((uintptr_t)p & 15) == 0) {
                if (MB == 1) {
                    const uint4 v = *(const uint4*)p;
                    sel[0] = lm_sel_bytes4(v.x), sel[1] = lm_sel_bytes4(v.y), sel[2] = lm_sel_bytes4(v.z), sel[3] = lm_sel_bytes4(v.w);
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q) sel[q] = lm_sel_f32x4(((const uint4*)p)[q], a.tkey);
                }
            } else {
                sel[0] = sel[1] = sel[2] = sel[3] = 0u;
#pragma unroll
                for (int i = 0; i < 16; ++i)
                    if (i < cnt && lm_set_at<MB>(p, i, a.tkey)) sel[i >> 2] |= 0xffu << (8 * (i & 3));
            }
            const unsigned id4 = (step >> 24) * 0x01010101u;
#pragma unroll
            for (int q = 0; q < 4; ++q) lab[q] = (id4 & sel[q]) | (lab[q] & ~sel[q]), painted[q] |= sel[q];
        }
        // colours: painted ? table[id] : 0, 16 triples packed into 48 bytes
        unsigned col[12] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const unsigned sh8 = 8 * (i & 3);
            const unsigned c = ((painted[i >> 2] >> sh8) & 1u) ? table[(lab[i >> 2] >> sh8) & 0xffu] : 0u;
            const int w = (24 * i) >> 5, sh = (24 * i) & 31;
            col[w] |= c << sh;
            if (sh > 8) col[w + 1] |= c >> (32 - sh);
        }
        const long o = f * a.HW + p0;
        unsigned char* idx = a.index + o;
        unsigned char* rgb = a.color + 3 * o;
        if (cnt == 16 && (o & 15) == 0) {              // index and color are 16-byte aligned: so are o and 3 o
            *(uint4*)idx = make_uint4(lab[0], lab[1], lab[2], lab[3]);
            ((uint4*)rgb)[0] = make_uint4(col[0], col[1], col[2], col[3]);
            ((uint4*)rgb)[1] = make_uint4(col[4], col[5], col[6], col[7]);
            ((uint4*)rgb)[2] = make_uint4(col[8], col[9], col[10], col[11]);
        } else {
#pragma unroll
            for (int i = 0; i < 16; ++i)
                if (i < cnt) idx[i] = (unsigned char)(lab[i >> 2] >> (8 * (i & 3)));
#pragma unroll
            for (int i = 0; i < 48; ++i)
                if (i < 3 * cnt) rgb[i] = (unsigned char)(col[i >> 2] >> (8 * (i & 3)));
        }
    }
}

int lm_check_masks(const char* who, int mask_bytes, int F, int n, int H, int W, long stride_f, long stride_n) {
    ORV_REQUIRE(F >= 0, "%s: F must not be negative (got %d)", who, F);
    ORV_REQUIRE(n >= 0 && n < LM_MAX_MASKS, "%s: n must not be negative and must be below 2^24 (got %d)", who, n);
    ORV_REQUIRE(H >= 1 && W >= 1 && H <= LM_MAX_DIM && W <= LM_MAX_DIM, "%s: the mask planes are %d x %d; supported: 1 <= H, W < 65536", who, H, W);
    ORV_REQUIRE(mask_bytes == 1 || mask_bytes == 4, "%s: mask_bytes = %d; supported: 1 (bool or uint8, set where nonzero) or 4 (fp32 logits)", who, mask_bytes);
    ORV_REQUIRE(stride_f >= 0 && stride_n >= 0 && stride_f < LM_MAX_STRIDE && stride_n < LM_MAX_STRIDE,
                "%s: the element strides of F and n are %ld and %ld; supported: 0 <= stride < 2^40", who, stride_f, stride_n);
    return ORV_OK;
}

int lm_threshold_key(float threshold) {
    unsigned b;
    memcpy(&b, &threshold, 4);
    return (b & 0x7fffffffu) > 0x7f800000u ? 0x7fffffff : lm_key(b);      // a NaN threshold: nothing is set
}

}  // namespace

extern "C" int orv_lm_mask_stats(const void* masks, int mask_bytes, int F, int n, int H, int W, long stride_f, long stride_n, float threshold,
                                 int bands, int* workspace, long* area, long* xyxy, void* stream) {
    if (int e = lm_check_masks("orv_lm_mask_stats", mask_bytes, F, n, H, W, stride_f, stride_n)) return e;
    ORV_REQUIRE(bands >= 1 && bands <= H, "orv_lm_mask_stats: bands = %d row bands per plane; supported: 1 to H = %d", bands, H);
    const long planes = (long)F * n;
    ORV_REQUIRE(planes * bands < 2147483648L, "orv_lm_mask_stats: F n bands = %ld workgroups; supported: below 2^31", planes * bands);
    if (planes == 0) return ORV_OK;
    ORV_REQUIRE(masks && workspace && area && xyxy, "orv_lm_mask_stats: null pointer (masks / workspace / area / xyxy)");
    ORV_REQUIRE(orv_aligned(masks, (uintptr_t)mask_bytes) && orv_aligned(workspace, 4) && orv_aligned(area, 8) && orv_aligned(xyxy, 8),
                "orv_lm_mask_stats: fp32 masks and the workspace must be 4-byte, area and xyxy 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int tkey = lm_threshold_key(threshold);
    const unsigned char* src = (const unsigned char*)masks;
    if (mask_bytes == 1)
        hipLaunchKernelGGL(lm_stats_kernel<1>, dim3((unsigned)(planes * bands)), dim3(256), 0, s, src, n, H, W, stride_f, stride_n, tkey, bands, workspace);
    else
        hipLaunchKernelGGL(lm_stats_kernel<4>, dim3((unsigned)(planes * bands)), dim3(256), 0, s, src, n, H, W, stride_f, stride_n, tkey, bands, workspace);
    hipLaunchKernelGGL(lm_stats_final_kernel, dim3(orv_blocks(planes, 256)), dim3(256), 0, s, workspace, planes, bands, area, xyxy);
    return orv_check_launch("orv_lm_mask_stats");
}

extern "C" int orv_lm_compose(const void* masks, int mask_bytes, int F, int n, int H, int W, long stride_f, long stride_n, float threshold,
                              const int* order, int m, const unsigned char* label_ids, const unsigned char* palette, unsigned* steps,
                              unsigned char* index, unsigned char* color, void* stream) {
    if (int e = lm_check_masks("orv_lm_compose", mask_bytes, F, n, H, W, stride_f, stride_n)) return e;
    ORV_REQUIRE(m >= 0 && m <= n, "orv_lm_compose: m = %d paint steps; supported: 0 to n = %d", m, n);
    ORV_REQUIRE(m == 0 || (order && label_ids), "orv_lm_compose: null pointer (order / label_ids, host arrays)");
    for (int k = 0; k < m; ++k)                                        // order is a host array; the device pointers are never followed
        ORV_REQUIRE(order[k] >= 0 && order[k] < n, "orv_lm_compose: order[%d] = %d; supported: distinct mask numbers in [0, n = %d)", k, order[k], n);
    if (F == 0) return ORV_OK;
    ORV_REQUIRE(palette, "orv_lm_compose: null pointer (palette, a host array of 60 triples)");
    ORV_REQUIRE(steps && index && color && (m == 0 || masks), "orv_lm_compose: null pointer (masks / steps / index / color)");
    ORV_REQUIRE(orv_aligned(masks, (uintptr_t)mask_bytes) && orv_aligned(steps, 4) && orv_aligned(index, 16) && orv_aligned(color, 16),
                "orv_lm_compose: fp32 masks and steps must be 4-byte, index and color 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    static thread_local std::vector<unsigned> host;                   // the steps and the id -> triple table, staged for one copy
    host.resize((size_t)m + LM_TABLE);
    for (int k = 0; k < m; ++k) host[k] = (unsigned)order[k] | (unsigned)label_ids[order[k]] << 24;
    for (int id = 0; id < LM_TABLE; ++id) {
        const unsigned char* c = palette + 3 * (id % 60);
        host[m + id] = (unsigned)c[0] | (unsigned)c[1] << 8 | (unsigned)c[2] << 16;
    }
    if (hipMemcpyAsync(steps, host.data(), host.size() * sizeof(unsigned), hipMemcpyHostToDevice, s) != hipSuccess) {
        orv_set_error("orv_lm_compose: the copy of the paint steps to the device failed: %s", hipGetErrorString(hipGetLastError()));
        return ORV_EINVAL;
    }
    LmComposeArgs a;
    a.masks = (const unsigned char*)masks, a.steps = steps, a.index = index, a.color = color;
    a.stride_f = stride_f, a.stride_n = stride_n, a.HW = (long)H * W, a.groups = (a.HW + 15) / 16, a.total = a.groups * F;
    a.m = m, a.tkey = lm_threshold_key(threshold);
    const long blocks = (a.total + 255) / 256;
    const unsigned grid = (unsigned)(blocks < LM_GRID_CAP ? blocks : LM_GRID_CAP);
    if (mask_bytes == 1)
        hipLaunchKernelGGL(lm_compose_kernel<1>, dim3(grid), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL(lm_compose_kernel<4>, dim3(grid), dim3(256), 0, s, a);
    return orv_check_launch("orv_lm_compose");
}
