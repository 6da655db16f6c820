// Fused CAME (confidence-guided Adam with factored second moments; FusedCAME) on the flat layout of the fused AdamW: every
// parameter a segment padded to 2048 elements, bf16 weights (+ the int16 low halves of orv_adamw_flat_ex mode 1), bf16 gradients, ONE fp32
// moment m per element.  The second moment of a parameter of shape [..., R, C] is a row vector and a column vector per R x C matrix
// (B = prod(shape[:-2]) matrices), that of a parameter of fewer than two dimensions an fp32 value per element (v).
//
// The rule, g the gradient times the clip coefficient, w the weight, all state fp32:
//      q = g g + eps1
//      factored:   r = b2 r + (1-b2) mean_j q ;  c = b2 c + (1-b2) mean_i q ;  u = (g rsqrt(r_i / mean_i r)) rsqrt(c_j)
//      otherwise:  v = b2 v + (1-b2) q ;  u = g rsqrt(v)
//      k = max(1, sqrt(mean of u u over the parameter) / clip_threshold) ;  u = u / k
//      m = b1 m + (1-b1) u ;  s = (u - m)^2 + eps2                                        (the new m)
//      factored:   Rr = b3 Rr + (1-b3) mean_j s ;  Cc = b3 Cc + (1-b3) mean_i s ;  out = (m rsqrt(Rr_i / mean_i Rr)) rsqrt(Cc_j)
//      otherwise:  out = m
//      w = w - (wd lr) w  (wd != 0) ;  w = w - lr out
//
// Work units.  A factored matrix is cut into tiles of 64 rows x 256 columns, one workgroup of 256 lanes each: lane (lr = t / 32, lc = t % 32)
// owns columns 8 lc .. 8 lc + 7 of rows lr, lr + 8, ..., lr + 56 of the tile - one 16-byte access per row where C % 8 == 0 (every row of the
// matrix is then 16-byte aligned), element accesses otherwise.  An unfactored parameter is cut into chunks of 2048 elements, 8 per lane.  The
// device table `geom` (12 int64 per segment: B, R, C, first tile, first matrix, offsets into the row / column statistics, into v, into the
// row / column partial sums, element count, 0; R == 0 marks an unfactored segment) maps a workgroup to its tile by a binary search.
//
// One step is seven stream-ordered launches (orv_came_launch, which = 0 .. 6; orv_came_step issues all of them):
//   0  sweep  reads g.        factored: the tile's row sums and column sums of q -> row_part / col_part.
//                             unfactored: v (read, written) and the chunk's sum of u u -> usq_part.
//   1  finish one workgroup per matrix: adds the partial sums of every row / column in ascending tile order in fp64, stores r and c (fp32),
//             mean_i r (fp64, over the stored values) and the factors rfac_i = 1 / sqrt(r_i / mean r), cfac_j = 1 / sqrt(c_j) (fp64, stored fp32).
//   2  sweep  reads g.        factored: the tile's sum of ((g rfac_i) cfac_j)^2 -> usq_part.
//   3  finish one workgroup per segment: adds its usq_part in fp64 -> k and the RMS of u (fp32 pair per segment).
//   4  sweep  reads g, m; writes m.   u = (g (rfac_i / k)) cfac_j  [unfactored: (g (1 / sqrt(v))) / k] ; m ; the tile's row / column sums of s.
//   5  finish as 1 on Rr, Cc with b3.
//   6  sweep  reads m, w; writes w.   mode 0: w is the bf16 weight, stored nearest-even; mode 1: the split fp32 master, stored by the rule of
//             orv_adamw_flat_ex mode 1.  The arithmetic is the same.
// Every sum has a fixed order - 8 values of a lane as a balanced tree, the 32 lanes of a row by xor-shuffles 1, 2, 4, 8, 16, the 8 lane rows
// of a column as a balanced tree, tiles in ascending order - and nothing is accumulated atomically: two runs give identical bytes.  The scratch
// (fp32) holds, in this order: row_part [n_rowp], col_part [n_colp], usq_part [n_tiles], rfac [n_rows], cfac [n_cols], (k, rms) [2 nseg].
// Inactive segments, padding, and the elements of a chunk past the parameter's end keep every byte.
#include "common.hpp"

#pragma clang fp contract(off)

namespace {

enum { G_B = 0, G_R, G_C, G_TILE0, G_MAT0, G_ROW0, G_COL0, G_V0, G_RP0, G_CP0, G_NUMEL, G_STRIDE = 12 };
enum { TR = 64, TC = 256 };

struct Came {            // the kernel-side copy of orv_came_t with the scratch regions resolved
    bf16_t* p; int16_t* lo; const bf16_t* g; float* m;
    float *r, *c, *res_r, *res_c, *v;
    const long* seg_start; const uint8_t* active; int nseg;
    const long* geom;
    float *row_part, *col_part, *usq_part, *rfac, *cfac, *kbuf;
    const float* clip;
    float lr, b1, b2, b3, eps1, eps2, clip_threshold, wd;
};

// last segment whose first tile (field G_TILE0) or first matrix (G_MAT0) is <= x; segments that own nothing share their start with the
// owner behind them, which is the last one
__device__ __forceinline__ int owner_of(const long* __restrict__ geom, int nseg, int field, long x) {
    int lo = 0, hi = nseg - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (geom[(long)mid * G_STRIDE + field] <= x) lo = mid; else hi = mid - 1; }
    return lo;
}

struct Tile {
    int seg;
    long R, C;               // R == 0: a chunk of an unfactored segment
    long flat;               // factored: flat index of the matrix' element (0, 0); chunk: of its first element
    long i0, j0;             // first row of the tile; first column of this lane
    long rows, cols;         // index of row 0 / column 0 of the matrix in the row / column arrays (statistics and factors)
    long rowp, colp;         // index of row 0 / column 0 in this tile's slice of row_part / col_part
    long vi, left;           // chunk: index of this lane's first element in v; elements of the parameter from there on (may be <= 0)
    int nv;                  // factored: valid columns of this lane, 0 .. 8
    bool vec;
};

__device__ __forceinline__ Tile tile_of(const Came& a, long tile) {
    Tile t;
    t.seg = owner_of(a.geom, a.nseg, G_TILE0, tile);
    const long* gm = a.geom + (long)t.seg * G_STRIDE;
    const long local = tile - gm[G_TILE0];
    t.R = gm[G_R]; t.C = gm[G_C];
    if (t.R == 0) {
        const long e = local * 2048 + threadIdx.x * 8;
        t.flat = a.seg_start[t.seg] + e;
        t.vi = gm[G_V0] + e;
        t.left = gm[G_NUMEL] - e;
        t.vec = true; t.nv = 0; t.i0 = t.j0 = t.rows = t.cols = t.rowp = t.colp = 0;
        return t;
    }
    const long nct = (t.C + TC - 1) / TC, nrt = (t.R + TR - 1) / TR;
    const long b = local / (nrt * nct), rem = local % (nrt * nct), rt = rem / nct, ct = rem % nct;
    t.flat = a.seg_start[t.seg] + b * t.R * t.C;
    t.i0 = rt * TR;
    t.j0 = ct * TC + (threadIdx.x & 31) * 8;
    t.rows = gm[G_ROW0] + b * t.R;
    t.cols = gm[G_COL0] + b * t.C;
    t.rowp = gm[G_RP0] + (b * nct + ct) * t.R;
    t.colp = gm[G_CP0] + (b * nrt + rt) * t.C;
    const long nv = t.C - t.j0;
    t.nv = nv >= 8 ? 8 : nv > 0 ? (int)nv : 0;
    t.vec = (t.C & 7) == 0;
    t.vi = 0; t.left = 0;
    return t;
}

__device__ __forceinline__ void load8_bf16(const bf16_t* __restrict__ x, long off, int nv, bool vec, float out[8]) {
    if (vec && nv == 8) {
        const uint4 u = *(const uint4*)(x + off);
        const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) out[e] = __uint_as_float((e & 1) ? w[e >> 1] & 0xffff0000u : w[e >> 1] << 16);
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) out[e] = e < nv ? bf2f(x[off + e]) : 0.f;
    }
}

__device__ __forceinline__ void load8_f32(const float* __restrict__ x, long off, int nv, bool vec, float out[8]) {
    if (vec && nv == 8) {
        const float4 a = *(const float4*)(x + off), b = *(const float4*)(x + off + 4);
        out[0] = a.x; out[1] = a.y; out[2] = a.z; out[3] = a.w; out[4] = b.x; out[5] = b.y; out[6] = b.z; out[7] = b.w;
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) out[e] = e < nv ? x[off + e] : 0.f;
    }
}

__device__ __forceinline__ void store8_f32(float* __restrict__ x, long off, int nv, bool vec, const float in[8]) {
    if (vec && nv == 8) {
        *(float4*)(x + off) = make_float4(in[0], in[1], in[2], in[3]);
        *(float4*)(x + off + 4) = make_float4(in[4], in[5], in[6], in[7]);
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) if (e < nv) x[off + e] = in[e];
    }
}

__device__ __forceinline__ float tree8(const float x[8]) { return ((x[0] + x[1]) + (x[2] + x[3])) + ((x[4] + x[5]) + (x[6] + x[7])); }

// the 32 lanes that share a row (lanes 32 h .. 32 h + 31 of a wave): every lane ends with the same sum, a fixed order
__device__ __forceinline__ float row_sum32(float x) {
#pragma unroll
    for (int s = 1; s < 32; s <<= 1) x += __shfl_xor(x, s, 32);
    return x;
}

// the workgroup's sum of one value per lane -> lane 0 (wave tree, then the four waves in order); red: 4 floats of LDS
__device__ __forceinline__ float block_sum(float x, float* red) {
    x = wave_sum_valu(x);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// Writes the tile's row sums and column sums of val[jj][e] (row i0 + 8 jj + lr, column j0 + e; zeros where there is no element).
__device__ __forceinline__ void tile_row_col_sums(const Came& a, const Tile& t, const float (&val)[8][8], float (*red)[TC]) {
    const int lr = threadIdx.x >> 5, lc = threadIdx.x & 31;
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) {
        const float rs = row_sum32(tree8(val[jj]));
        const long i = t.i0 + jj * 8 + lr;
        if (lc == 0 && i < t.R) a.row_part[t.rowp + i] = rs;
    }
    float cs[8];
#pragma unroll
    for (int e = 0; e < 8; ++e)
        cs[e] = ((val[0][e] + val[1][e]) + (val[2][e] + val[3][e])) + ((val[4][e] + val[5][e]) + (val[6][e] + val[7][e]));
    *(float4*)&red[lr][lc * 8] = make_float4(cs[0], cs[1], cs[2], cs[3]);
    *(float4*)&red[lr][lc * 8 + 4] = make_float4(cs[4], cs[5], cs[6], cs[7]);
    __syncthreads();
    const int x = threadIdx.x;
    const long j = t.j0 - lc * 8 + x;            // the tile's first column + x
    const float sum = ((red[0][x] + red[1][x]) + (red[2][x] + red[3][x])) + ((red[4][x] + red[5][x]) + (red[6][x] + red[7][x]));
    if (j < t.C) a.col_part[t.colp + j] = sum;
}

// ---- launch 0: q sums (factored) ; v and the sum of u u (unfactored) ----
__global__ __launch_bounds__(256) void came_sweep_q(const Came a) {
    __shared__ float red[8][TC];
    const Tile t = tile_of(a, blockIdx.x);
    if (!a.active[t.seg]) return;
    const float cl = a.clip ? *a.clip : 1.f;
    if (t.R == 0) {
        float g[8], v[8], uu[8];
        load8_bf16(a.g, t.flat, 8, true, g);
        load8_f32(a.v, t.vi, 8, true, v);
        const float omb2 = 1.f - a.b2;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            uu[e] = 0.f;
            if (e < t.left) {
                const float gr = g[e] * cl;
                v[e] = a.b2 * v[e] + omb2 * (gr * gr + a.eps1);
                const float u = gr * (1.f / sqrtf(v[e]));
                uu[e] = u * u;
            }
        }
        store8_f32(a.v, t.vi, 8, true, v);
        const float s = block_sum(tree8(uu), &red[0][0]);
        if (threadIdx.x == 0) a.usq_part[blockIdx.x] = s;
        return;
    }
    const int lr = threadIdx.x >> 5;
    float q[8][8];
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) {
        const long i = t.i0 + jj * 8 + lr;
        float g[8];
        const int nv = i < t.R ? t.nv : 0;
        load8_bf16(a.g, t.flat + i * t.C + t.j0, nv, t.vec, g);
#pragma unroll
        for (int e = 0; e < 8; ++e) { const float gr = g[e] * cl; q[jj][e] = e < nv ? gr * gr + a.eps1 : 0.f; }
    }
    tile_row_col_sums(a, t, q, red);
}

// ---- launches 1 and 5: one workgroup per matrix ----
__global__ __launch_bounds__(256) void came_finish_stats(const Came a, float* __restrict__ sr, float* __restrict__ sc, float beta) {
    __shared__ double red[256];
    const int seg = owner_of(a.geom, a.nseg, G_MAT0, blockIdx.x);
    if (!a.active[seg]) return;
    const long* gm = a.geom + (long)seg * G_STRIDE;
    const long R = gm[G_R], C = gm[G_C], b = blockIdx.x - gm[G_MAT0];
    const long nct = (C + TC - 1) / TC, nrt = (R + TR - 1) / TR;
    const long rows = gm[G_ROW0] + b * R, cols = gm[G_COL0] + b * C;
    const double bt = (double)beta, omb = 1.0 - (double)beta;
    double lsum = 0.0;
    for (long i = threadIdx.x; i < R; i += 256) {
        double s = 0.0;
        for (long ct = 0; ct < nct; ++ct) s += (double)a.row_part[gm[G_RP0] + (b * nct + ct) * R + i];
        const float rn = (float)(bt * (double)sr[rows + i] + omb * (s / (double)C));
        sr[rows + i] = rn;
        lsum += (double)rn;
    }
    red[threadIdx.x] = lsum;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
        __syncthreads();
    }
    const double mean = red[0] / (double)R;
    for (long i = threadIdx.x; i < R; i += 256)          // the values this lane stored above
        a.rfac[rows + i] = (float)(1.0 / sqrt((double)sr[rows + i] / mean));
    for (long j = threadIdx.x; j < C; j += 256) {
        double s = 0.0;
        for (long rt = 0; rt < nrt; ++rt) s += (double)a.col_part[gm[G_CP0] + (b * nrt + rt) * C + j];
        const float cn = (float)(bt * (double)sc[cols + j] + omb * (s / (double)R));
        sc[cols + j] = cn;
        a.cfac[cols + j] = (float)(1.0 / sqrt((double)cn));
    }
}

// ---- launch 2: the tile's sum of u u before the division by k ----
__global__ __launch_bounds__(256) void came_sweep_usq(const Came a) {
    __shared__ float red[4];
    const Tile t = tile_of(a, blockIdx.x);
    if (!a.active[t.seg] || t.R == 0) return;
    const float cl = a.clip ? *a.clip : 1.f;
    const int lr = threadIdx.x >> 5;
    float cf[8], part[8];
    load8_f32(a.cfac, t.cols + t.j0, t.nv, false, cf);
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) {
        const long i = t.i0 + jj * 8 + lr;
        const int nv = i < t.R ? t.nv : 0;
        float g[8], uu[8];
        load8_bf16(a.g, t.flat + i * t.C + t.j0, nv, t.vec, g);
        const float rf = i < t.R ? a.rfac[t.rows + i] : 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) { const float u = ((g[e] * cl) * rf) * cf[e]; uu[e] = e < nv ? u * u : 0.f; }
        part[jj] = tree8(uu);
    }
    const float s = block_sum(tree8(part), red);
    if (threadIdx.x == 0) a.usq_part[blockIdx.x] = s;
}

// ---- launch 3: one workgroup per segment -> (k, rms) ----
__global__ __launch_bounds__(256) void came_finish_k(const Came a, long n_tiles) {
    __shared__ double red[256];
    const int seg = blockIdx.x;
    if (!a.active[seg]) return;
    const long* gm = a.geom + (long)seg * G_STRIDE;
    const long t0 = gm[G_TILE0], t1 = seg + 1 < a.nseg ? gm[G_STRIDE + G_TILE0] : n_tiles;
    double s = 0.0;
    for (long t = t0 + threadIdx.x; t < t1; t += 256) s += (double)a.usq_part[t];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const double rms = sqrt(red[0] / (double)gm[G_NUMEL]);
    a.kbuf[2 * seg] = (float)fmax(1.0, rms / (double)a.clip_threshold);
    a.kbuf[2 * seg + 1] = (float)rms;
}

// ---- launch 4: m and the sums of s ----
__global__ __launch_bounds__(256) void came_sweep_m(const Came a) {
    __shared__ float red[8][TC];
    const Tile t = tile_of(a, blockIdx.x);
    if (!a.active[t.seg]) return;
    const float cl = a.clip ? *a.clip : 1.f, k = a.kbuf[2 * t.seg], omb1 = 1.f - a.b1;
    if (t.R == 0) {
        float g[8], v[8], m[8];
        load8_bf16(a.g, t.flat, 8, true, g);
        load8_f32(a.v, t.vi, 8, true, v);
        load8_f32(a.m, t.flat, 8, true, m);
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (e < t.left) m[e] = a.b1 * m[e] + omb1 * (((g[e] * cl) * (1.f / sqrtf(v[e]))) / k);
        store8_f32(a.m, t.flat, 8, true, m);
        return;
    }
    const int lr = threadIdx.x >> 5;
    float cf[8], s[8][8];
    load8_f32(a.cfac, t.cols + t.j0, t.nv, false, cf);
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) {
        const long i = t.i0 + jj * 8 + lr, off = t.flat + i * t.C + t.j0;
        const int nv = i < t.R ? t.nv : 0;
        float g[8], m[8];
        load8_bf16(a.g, off, nv, t.vec, g);
        load8_f32(a.m, off, nv, t.vec, m);
        const float rfk = i < t.R ? a.rfac[t.rows + i] / k : 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float u = ((g[e] * cl) * rfk) * cf[e];
            m[e] = a.b1 * m[e] + omb1 * u;
            const float d = u - m[e];
            s[jj][e] = e < nv ? d * d + a.eps2 : 0.f;
        }
        store8_f32(a.m, off, nv, t.vec, m);
    }
    tile_row_col_sums(a, t, s, red);
}

// ---- launch 6: the weight update ----
__device__ __forceinline__ uint32_t half_of(const uint32_t* w, int e) { return (e & 1) ? w[e >> 1] >> 16 : w[e >> 1] & 0xffffu; }

// 8 weights at `off` (nv valid): w = w - (wd lr) w ; w = w - lr out.  MODE 0: bf16 weight, nearest-even store; MODE 1: split fp32 master.
template <int MODE>
__device__ __forceinline__ void update8(const Came& a, long off, int nv, bool vec, const float out[8]) {
    uint32_t pb[8], lb[8];
    if (vec && nv == 8) {
        const uint4 up = *(const uint4*)(a.p + off);
        const uint32_t wp[4] = {up.x, up.y, up.z, up.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) { pb[e] = half_of(wp, e); lb[e] = 0u; }
        if (MODE == 1) {
            const uint4 ul = *(const uint4*)(a.lo + off);
            const uint32_t wl[4] = {ul.x, ul.y, ul.z, ul.w};
#pragma unroll
            for (int e = 0; e < 8; ++e) lb[e] = half_of(wl, e);
        }
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            pb[e] = e < nv ? a.p[off + e] : 0u;
            lb[e] = (MODE == 1 && e < nv) ? (uint32_t)(uint16_t)a.lo[off + e] : 0u;
        }
    }
    const float wdlr = a.wd * a.lr;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        float w = __uint_as_float((pb[e] << 16) + (uint32_t)(int32_t)(int16_t)lb[e]);
        if (a.wd != 0.f) w = w - wdlr * w;
        w = w - a.lr * out[e];
        const uint32_t u = __float_as_uint(w), ab = u & 0x7fffffffu;
        if (MODE == 0) {
            pb[e] = f2bf(w);
        } else if (ab >= 0x7f800000u) {          // infinity / NaN: the matching bf16 (NaN kept quiet), no low half
            pb[e] = (u >> 16) | (ab > 0x7f800000u ? 0x40u : 0u);
            lb[e] = 0u;
        } else {
            pb[e] = (u + 0x8000u) >> 16;
            lb[e] = (u - (pb[e] << 16)) & 0xffffu;
        }
    }
    if (vec && nv == 8) {
        *(uint4*)(a.p + off) = make_uint4(pb[0] | pb[1] << 16, pb[2] | pb[3] << 16, pb[4] | pb[5] << 16, pb[6] | pb[7] << 16);
        if (MODE == 1)
            *(uint4*)(a.lo + off) = make_uint4(lb[0] | lb[1] << 16, lb[2] | lb[3] << 16, lb[4] | lb[5] << 16, lb[6] | lb[7] << 16);
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (e < nv) {
                a.p[off + e] = (bf16_t)pb[e];
                if (MODE == 1) a.lo[off + e] = (int16_t)lb[e];
            }
    }
}

template <int MODE>
__global__ __launch_bounds__(256) void came_sweep_w(const Came a) {
    const Tile t = tile_of(a, blockIdx.x);
    if (!a.active[t.seg]) return;
    if (t.R == 0) {
        const int nv = t.left >= 8 ? 8 : t.left > 0 ? (int)t.left : 0;
        float m[8];
        load8_f32(a.m, t.flat, 8, true, m);
        update8<MODE>(a, t.flat, nv, true, m);
        return;
    }
    const int lr = threadIdx.x >> 5;
    float cf[8];
    load8_f32(a.cfac, t.cols + t.j0, t.nv, false, cf);
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) {
        const long i = t.i0 + jj * 8 + lr, off = t.flat + i * t.C + t.j0;
        const int nv = i < t.R ? t.nv : 0;
        float m[8], out[8];
        load8_f32(a.m, off, nv, t.vec, m);
        const float rf = i < t.R ? a.rfac[t.rows + i] : 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) out[e] = (m[e] * rf) * cf[e];
        update8<MODE>(a, off, nv, t.vec, out);
    }
}

}  // namespace

extern "C" int orv_came_launch(const orv_came_t* d, int which, void* stream) {
    ORV_REQUIRE(d, "orv_came_launch: bad arguments (a null descriptor)");
    ORV_REQUIRE(which >= 0 && which <= 6, "orv_came_launch: which=%d (0 .. 6: q sums, statistics, u u sums, k, m and s sums, confidence, weights)", which);
    ORV_REQUIRE(d->mode == 0 || d->mode == 1, "orv_came_launch: mode=%d (0 bf16, 1 split_fp32)", d->mode);
    ORV_REQUIRE(d->p && d->g && d->m && d->seg_start && d->seg_active && d->geom && d->scratch && d->nseg > 0,
                "orv_came_launch: bad arguments (a null buffer, or nseg=%d)", d->nseg);
    ORV_REQUIRE(d->mode != 1 || d->lo, "orv_came_launch: mode 1 (split_fp32) needs the low-half buffer lo (a null buffer)");
    ORV_REQUIRE(d->n > 0 && d->n % 2048 == 0, "orv_came_launch: n=%ld must be a multiple of 2048 (pad every segment)", d->n);
    ORV_REQUIRE(d->n_rows >= 0 && d->n_cols >= 0 && d->n_v >= 0 && d->n_v % 2048 == 0 && d->n_rowp >= 0 && d->n_colp >= 0 && d->n_mats >= 0,
                "orv_came_launch: bad sizes (n_rows=%ld n_cols=%ld n_v=%ld n_rowp=%ld n_colp=%ld n_mats=%ld)", d->n_rows, d->n_cols, d->n_v,
                d->n_rowp, d->n_colp, d->n_mats);
    ORV_REQUIRE(d->n_tiles > 0 && d->n_tiles < (1L << 31) && d->n_mats < (1L << 31), "orv_came_launch: n_tiles=%ld must lie in [1, 2^31)", d->n_tiles);
    ORV_REQUIRE((d->n_mats == 0) == (d->n_rows == 0) && (d->n_mats == 0) == (d->n_cols == 0),
                "orv_came_launch: n_mats=%ld, n_rows=%ld and n_cols=%ld must be zero together", d->n_mats, d->n_rows, d->n_cols);
    ORV_REQUIRE(d->n_rows == 0 || (d->r && d->c && d->res_r && d->res_c), "orv_came_launch: factored segments need r, c, res_r, res_c (a null buffer)");
    ORV_REQUIRE(d->n_v == 0 || d->v, "orv_came_launch: unfactored segments need v (a null buffer)");
    const long need = d->n_rowp + d->n_colp + d->n_tiles + d->n_rows + d->n_cols + 2L * d->nseg;
    ORV_REQUIRE(d->n_scratch >= need, "orv_came_launch: scratch holds %ld floats, the layout needs %ld", d->n_scratch, need);
    ORV_REQUIRE(d->eps1 > 0.f, "orv_came_launch: eps1=%g must be greater than 0 (a zero gradient divides by it)", (double)d->eps1);
    ORV_REQUIRE(d->clip_threshold > 0.f, "orv_came_launch: clip_threshold=%g must be greater than 0", (double)d->clip_threshold);
    Came a;
    a.p = (bf16_t*)d->p; a.lo = (int16_t*)d->lo; a.g = (const bf16_t*)d->g; a.m = d->m;
    a.r = d->r; a.c = d->c; a.res_r = d->res_r; a.res_c = d->res_c; a.v = d->v;
    a.seg_start = d->seg_start; a.active = d->seg_active; a.nseg = d->nseg; a.geom = d->geom;
    a.row_part = d->scratch; a.col_part = a.row_part + d->n_rowp; a.usq_part = a.col_part + d->n_colp;
    a.rfac = a.usq_part + d->n_tiles; a.cfac = a.rfac + d->n_rows; a.kbuf = a.cfac + d->n_cols;
    a.clip = d->clip_coef;
    a.lr = d->lr; a.b1 = d->beta1; a.b2 = d->beta2; a.b3 = d->beta3; a.eps1 = d->eps1; a.eps2 = d->eps2;
    a.clip_threshold = d->clip_threshold; a.wd = d->weight_decay;
    const dim3 tiles((unsigned)d->n_tiles), mats((unsigned)d->n_mats), block(256);
    hipStream_t st = (hipStream_t)stream;
    switch (which) {
    case 0: hipLaunchKernelGGL(came_sweep_q, tiles, block, 0, st, a); break;
    case 1: if (d->n_mats) hipLaunchKernelGGL(came_finish_stats, mats, block, 0, st, a, a.r, a.c, a.b2); break;
    case 2: if (d->n_mats) hipLaunchKernelGGL(came_sweep_usq, tiles, block, 0, st, a); break;
    case 3: hipLaunchKernelGGL(came_finish_k, dim3((unsigned)d->nseg), block, 0, st, a, d->n_tiles); break;
    case 4: hipLaunchKernelGGL(came_sweep_m, tiles, block, 0, st, a); break;
    case 5: if (d->n_mats) hipLaunchKernelGGL(came_finish_stats, mats, block, 0, st, a, a.res_r, a.res_c, a.b3); break;
    default:
        if (d->mode == 1) hipLaunchKernelGGL(came_sweep_w<1>, tiles, block, 0, st, a);
        else hipLaunchKernelGGL(came_sweep_w<0>, tiles, block, 0, st, a);
    }
    return orv_check_launch("orv_came_launch");
}

extern "C" int orv_came_step(const orv_came_t* d, void* stream) {
    for (int which = 0; which <= 6; ++which) {
        const int rc = orv_came_launch(d, which, stream);
        if (rc) return rc;
    }
    return 0;
}
