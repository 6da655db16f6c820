// Point-cloud cleaning and normals in front of ORV's reconstruction stage (the reference runs them per frame on the CPU through Open3D's
// KD-tree: _preprocess_points, orv/dataset/prepare_dataset.py:806-822, and process_nksr._preprocess_point_cloud, :729-741).
// Written from the arithmetic contract in DESIGN.md §17 (restated in include/orv_mi355.h): an exact k-nearest-neighbour search under the
// order (d2, index), the statistical outlier removal and the PCA normals on top of it.  The search is a uniform grid around a stable sort
// (torch): one clamped cell key per point, the sorted keys give a dense table of cell starts and the points in cell order, one wave per
// query walks the cubes of cells around the query's cell with its running list one entry per lane, and a query the walk cannot finish is
// scanned against every point by one workgroup.  Both kernels apply the same rule to the same fp64 distances, so the result is exact for
// every input and every cell edge.  No atomics anywhere and every reduction in a fixed order: bit-reproducible.
#include "common.hpp"
#include <math.h>

// the contract rounds every fp64 product and sum on its own: no contraction into an FMA anywhere in this file
#pragma clang fp contract(off)

namespace {

constexpr int PC_KMAX = 64;                    // the list lives one entry per lane
constexpr int PC_RMAX = 3;                     // rings of cells walked before a query is left to the brute kernel: 7 x 7 rows <= 64 lanes
constexpr int PC_NONE = 0x7fffffff;            // index of an empty list entry: sorts behind every point at d2 = +inf
constexpr long PC_MAX_CELLS = 1L << 24;
constexpr int PC_CHUNK = 1024;                 // points per workgroup of the outlier reductions

struct PcGrid {
    double lo[3], h;
    int g[3];                                  // cells along x, y, z
};

// floor((p - lo) / h) in fp64, clamped to the axis: a point outside the grid (and a NaN) lands in a border cell
__device__ __forceinline__ int pc_cell(float p, double lo, double h, int g) {
    const double t = floor(((double)p - lo) / h);
    if (!(t >= 1.0)) return 0;
    return t < (double)g ? (int)t : g - 1;
}

__device__ __forceinline__ double pc_d2(float qx, float qy, float qz, float px, float py, float pz) {
    const double dx = (double)px - (double)qx, dy = (double)py - (double)qy, dz = (double)pz - (double)qz;
    return (dx * dx + dy * dy) + dz * dz;
}

// (d, i) < (e, j) in lexicographic order
__device__ __forceinline__ bool pc_less(double d, int i, double e, int j) { return d < e || (d == e && i < j); }

// The wave's list: lane r holds the entry of rank r, ascending in (d2, index), empty entries (+inf, PC_NONE) behind.  Every lane offers one
// candidate (or none): those below the entry of rank kk - 1 are found by ballot and inserted one by one, the entries behind the insertion
// point moving up one lane.  Called by all 64 lanes of a wave together.
__device__ __forceinline__ void pc_offer(double& ld, int& li, double cd, int ci, bool valid, int kk, int lane) {
    double kd = __shfl(ld, kk - 1, 64);
    int ki = __shfl(li, kk - 1, 64);
    unsigned long long m = __ballot(valid && pc_less(cd, ci, kd, ki));
    while (m) {
        const int l = __ffsll(m) - 1;
        m &= m - 1;
        const double d = __shfl(cd, l, 64);
        const int i = __shfl(ci, l, 64);
        if (!pc_less(d, i, kd, ki)) continue;                                  // the bar has moved since the ballot
        const int pos = __popcll(__ballot(pc_less(ld, li, d, i)));              // the list is sorted: the smaller entries are a prefix
        const double ud = __shfl_up(ld, 1, 64);
        const int ui = __shfl_up(li, 1, 64);
        if (lane == pos) ld = d, li = i;
        else if (lane > pos) ld = ud, li = ui;
        kd = __shfl(ld, kk - 1, 64);
        ki = __shfl(li, kk - 1, 64);
    }
}

// one thread per point: the linear key of its clamped cell
__global__ __launch_bounds__(256) void pc_cells_kernel(const float* __restrict__ points, int N, const PcGrid gr, long* __restrict__ keys) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const float* p = points + 3 * (long)i;
    const int cx = pc_cell(p[0], gr.lo[0], gr.h, gr.g[0]), cy = pc_cell(p[1], gr.lo[1], gr.h, gr.g[1]), cz = pc_cell(p[2], gr.lo[2], gr.h, gr.g[2]);
    keys[i] = ((long)cz * gr.g[1] + cy) * gr.g[0] + cx;
}

// thread t < n_cells + 1: start[t] = first sorted position whose key is >= t (binary search; start[n_cells] = N);
// thread t < N: the point of sorted entry t copied behind it, so that a cell's points are contiguous
__global__ __launch_bounds__(256) void pc_cell_table_kernel(const long* __restrict__ keys, const long* __restrict__ order,
                                                            const float* __restrict__ points, int N, int n_cells, int* __restrict__ start,
                                                            float* __restrict__ sorted_points) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t <= n_cells) {
        int lo = 0, hi = N;
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if (keys[mid] < t) lo = mid + 1;
            else hi = mid;
        }
        start[t] = lo;
    }
    if (t < N) {
        const unsigned long p = (unsigned long)order[t];
        float x = 0.0f, y = 0.0f, z = 0.0f;
        if (p < (unsigned long)N) x = points[3 * p], y = points[3 * p + 1], z = points[3 * p + 2];
        sorted_points[3 * t] = x, sorted_points[3 * t + 1] = y, sorted_points[3 * t + 2] = z;
    }
}

struct PcKnnArgs {
    const float* sorted_points;
    const long* order;
    const int* start;
    int* idx;
    double* d2;
    unsigned char* pending;
    PcGrid gr;
    int N, kk;
};

// the sorted entries [b, e) offered to the list, 64 at a time
__device__ __forceinline__ void pc_scan(const PcKnnArgs& a, float qx, float qy, float qz, int b, int e, double& ld, int& li, int lane) {
    unsigned long long m = __ballot(e > b);
    while (m) {
        const int l = __ffsll(m) - 1;
        m &= m - 1;
        const int B = __shfl(b, l, 64), E = __shfl(e, l, 64);
        for (int base = B; base < E; base += 64) {
            const int j = base + lane;
            const bool valid = j < E;
            double cd = 0.0;
            int ci = PC_NONE;
            if (valid) {
                const float* p = a.sorted_points + 3 * (long)j;
                cd = pc_d2(qx, qy, qz, p[0], p[1], p[2]);
                ci = (int)a.order[j];
            }
            pc_offer(ld, li, cd, ci, valid, a.kk, lane);
        }
    }
}

// One wave per query, the queries in cell order.  Ring r is the shell of the cube of (2r + 1)^3 cells around the query's cell: a lane
// takes one (y, z) row of the cube, whose cells are contiguous in the sorted order - the whole row on the shell's four sides, else its
// two end cells.  After ring r the walk stops when the list is full and its last d2 is below the squared distance to every face of the
// cube that is not on the grid's border (cells on the border are unbounded outwards); the distance is shrunk by 2^-40 of its operands,
// far above the rounding of the cell arithmetic, so a stop is never early.
__global__ __launch_bounds__(256) void pc_knn_kernel(const PcKnnArgs a) {
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);                         // wave-uniform
    if (q >= a.N) return;
    const unsigned long row = (unsigned long)a.order[q];
    if (row >= (unsigned long)a.N) return;
    const float qx = a.sorted_points[3 * (long)q], qy = a.sorted_points[3 * (long)q + 1], qz = a.sorted_points[3 * (long)q + 2];
    const PcGrid& gr = a.gr;
    const int gx = gr.g[0], gy = gr.g[1], gz = gr.g[2];
    const int cx = pc_cell(qx, gr.lo[0], gr.h, gx), cy = pc_cell(qy, gr.lo[1], gr.h, gy), cz = pc_cell(qz, gr.lo[2], gr.h, gz);
    const double u[3] = {(double)qx - gr.lo[0], (double)qy - gr.lo[1], (double)qz - gr.lo[2]};
    const int c[3] = {cx, cy, cz};

    double ld = (double)INFINITY;
    int li = PC_NONE;
    bool done = false;
    for (int r = 0; r <= PC_RMAX && !done; ++r) {
        const int side = 2 * r + 1;
        int b0 = 0, e0 = 0, b1 = 0, e1 = 0;
        if (lane < side * side) {
            const int dz = lane / side - r, dy = lane % side - r;
            const int y = cy + dy, z = cz + dz;
            if (y >= 0 && y < gy && z >= 0 && z < gz) {
                const int base = (z * gy + y) * gx;
                const int xl = cx - r, xh = cx + r;
                const int ady = dy < 0 ? -dy : dy, adz = dz < 0 ? -dz : dz;
                if ((ady > adz ? ady : adz) == r) {
                    b0 = a.start[base + (xl > 0 ? xl : 0)], e0 = a.start[base + (xh < gx - 1 ? xh : gx - 1) + 1];
                } else {
                    if (xl >= 0) b0 = a.start[base + xl], e0 = a.start[base + xl + 1];
                    if (xh < gx) b1 = a.start[base + xh], e1 = a.start[base + xh + 1];
                }
                b0 = b0 > 0 ? b0 : 0, b1 = b1 > 0 ? b1 : 0;
                e0 = e0 < a.N ? e0 : a.N, e1 = e1 < a.N ? e1 : a.N;
            }
        }
        pc_scan(a, qx, qy, qz, b0, e0, ld, li, lane);
        pc_scan(a, qx, qy, qz, b1, e1, ld, li, lane);

        double bound = (double)INFINITY;
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            const int cl = c[ax] - r, ch = c[ax] + r;
            if (cl > 0) {
                const double face = (double)cl * gr.h;
                const double gap = (u[ax] - face) - (fabs(u[ax]) + face) * 0x1p-40;
                bound = gap < bound ? gap : bound;
            }
            if (ch < gr.g[ax] - 1) {
                const double face = (double)(ch + 1) * gr.h;
                const double gap = (face - u[ax]) - (fabs(u[ax]) + face) * 0x1p-40;
                bound = gap < bound ? gap : bound;
            }
        }
        const double kd = __shfl(ld, a.kk - 1, 64);
        const int ki = __shfl(li, a.kk - 1, 64);
        done = ki != PC_NONE && (bound == (double)INFINITY || (bound > 0.0 && kd < bound * bound));
    }
    if (done && lane < a.kk) a.idx[row * a.kk + lane] = li, a.d2[row * a.kk + lane] = ld;
    if (lane == 0) a.pending[row] = done ? 0 : 1;
}

// One workgroup per listed query: every wave scans a quarter of the points, in index order, into a list of its own, and wave 0 merges the
// four lists through LDS.  The same (d2, index) rule as the grid walk, over all N points.
__global__ __launch_bounds__(256) void pc_knn_brute_kernel(const float* __restrict__ points, int N, int kk, const long* __restrict__ queries,
                                                           int* __restrict__ idx, double* __restrict__ d2) {
    __shared__ double s_d[4][64];
    __shared__ int s_i[4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long row = (unsigned long)queries[blockIdx.x];              // uniform over the workgroup
    if (row >= (unsigned long)N) return;
    const float qx = points[3 * row], qy = points[3 * row + 1], qz = points[3 * row + 2];
    double ld = (double)INFINITY;
    int li = PC_NONE;
    for (long base = (long)w * 64; base < N; base += 256) {
        const long j = base + lane;
        const bool valid = j < N;
        double cd = 0.0;
        if (valid) cd = pc_d2(qx, qy, qz, points[3 * j], points[3 * j + 1], points[3 * j + 2]);
        pc_offer(ld, li, cd, (int)j, valid, kk, lane);
    }
    s_d[w][lane] = ld, s_i[w][lane] = li;
    __syncthreads();
    if (w != 0) return;
    for (int o = 1; o < 4; ++o) pc_offer(ld, li, s_d[o][lane], s_i[o][lane], s_i[o][lane] != PC_NONE, kk, lane);
    if (lane < kk) idx[row * kk + lane] = li, d2[row * kk + lane] = ld;
}

// one thread per point: avg = (sum over the ranks, in rank order, of sqrt(d2)) / kk
__global__ __launch_bounds__(256) void pc_avg_kernel(const double* __restrict__ d2, int N, int kk, double* __restrict__ avg) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const double* row = d2 + (long)i * kk;
    double s = 0.0;
    for (int r = 0; r < kk; ++r) s = s + sqrt(row[r]);
    avg[i] = s / (double)kk;
}

__device__ __forceinline__ double pc_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// lanes by the xor butterfly, then the four waves in order: a fixed order, the same on every run; the sum is valid in thread 0
__device__ __forceinline__ double pc_block_sum(double v, double* red) {
    v = pc_wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// stage one of both reductions.  A workgroup owns PC_CHUNK consecutive points, a thread four of them in index order; over the points with
// avg > 0, partials[2 b] = their number and partials[2 b + 1] = the sum of avg (stats == NULL) or of (avg - mean)^2 (mean = stats[0])
__global__ __launch_bounds__(256) void pc_partial_kernel(const double* __restrict__ avg, int N, const double* __restrict__ stats,
                                                         double* __restrict__ partials) {
    __shared__ double red[4];
    const double mean = stats ? stats[0] : 0.0;
    double cnt = 0.0, s = 0.0;
    const long first = (long)blockIdx.x * PC_CHUNK + threadIdx.x * 4;
    for (int e = 0; e < 4; ++e) {
        const long i = first + e;
        if (i < N) {
            const double v = avg[i];
            if (v > 0.0) {
                const double t = stats ? (v - mean) * (v - mean) : v;
                cnt = cnt + 1.0, s = s + t;
            }
        }
    }
    cnt = pc_block_sum(cnt, red);
    s = pc_block_sum(s, red);
    if (threadIdx.x == 0) partials[2 * (long)blockIdx.x] = cnt, partials[2 * (long)blockIdx.x + 1] = s;
}

// stage two, one workgroup: thread t sums the partials t, t + 256, ... in order.  second == 0: stats[0] = mean = sum / V, stats[3] = V;
// second == 1: stats[1] = std = sqrt(sum / (V - 1)), stats[2] = thr = mean + std_ratio * std.  V == 0 gives mean = NaN, V == 1 std = NaN.
__global__ __launch_bounds__(256) void pc_final_kernel(const double* __restrict__ partials, int n_blocks, int second, double std_ratio,
                                                       double* __restrict__ stats) {
    __shared__ double red[4];
    double cnt = 0.0, s = 0.0;
    for (int b = threadIdx.x; b < n_blocks; b += 256) cnt = cnt + partials[2 * (long)b], s = s + partials[2 * (long)b + 1];
    cnt = pc_block_sum(cnt, red);
    s = pc_block_sum(s, red);
    if (threadIdx.x != 0) return;
    if (!second) {
        stats[0] = s / cnt, stats[3] = cnt;
    } else {
        const double sd = sqrt(s / (cnt - 1.0));
        stats[1] = sd, stats[2] = stats[0] + std_ratio * sd;
    }
}

__global__ __launch_bounds__(256) void pc_mask_kernel(const double* __restrict__ avg, int N, const double* __restrict__ stats,
                                                      unsigned char* __restrict__ keep) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const double v = avg[i], thr = stats[2];
    keep[i] = (v > 0.0 && v < thr) ? 1 : 0;
}

// A unit eigenvector of the smallest eigenvalue of the symmetric C = [[c00 c01 c02] [. c11 c12] [. . c22]], or (0, 0, 1) for C == 0.
// C is scaled by its largest |entry|; the eigenvalue comes from the trigonometric solution of the characteristic cubic; the eigenvector is
// the largest of the three cross products of the rows of M = C - lambda I (the columns of adj(M), which for a simple eigenvalue is a
// multiple of v v^T: a step of inverse iteration without a division).  When all three are below 1e-7 M has rank <= 1 (a double smallest
// eigenvalue: collinear neighbours): with u the row of M of largest norm (the line), the result is e x u normalised, e the coordinate
// axis of the smallest |u| component (the first such axis on a tie); M == 0 gives (0, 0, 1).
__device__ __forceinline__ void pc_min_eigenvector(double c00, double c01, double c02, double c11, double c12, double c22, double n[3]) {
    n[0] = 0.0, n[1] = 0.0, n[2] = 1.0;
    double s = fabs(c00);
    s = fmax(s, fabs(c01)), s = fmax(s, fabs(c02)), s = fmax(s, fabs(c11)), s = fmax(s, fabs(c12)), s = fmax(s, fabs(c22));
    if (!(s > 0.0)) return;
    const double a00 = c00 / s, a01 = c01 / s, a02 = c02 / s, a11 = c11 / s, a12 = c12 / s, a22 = c22 / s;
    const double q = (a00 + a11 + a22) / 3.0;
    const double p1 = a01 * a01 + a02 * a02 + a12 * a12;
    const double p2 = (a00 - q) * (a00 - q) + (a11 - q) * (a11 - q) + (a22 - q) * (a22 - q) + 2.0 * p1;
    const double p = sqrt(p2 / 6.0);
    double lam = q;
    if (p > 0.0) {
        const double b00 = (a00 - q) / p, b11 = (a11 - q) / p, b22 = (a22 - q) / p, b01 = a01 / p, b02 = a02 / p, b12 = a12 / p;
        double hdet = (b00 * (b11 * b22 - b12 * b12) - b01 * (b01 * b22 - b12 * b02) + b02 * (b01 * b12 - b11 * b02)) / 2.0;
        hdet = hdet < -1.0 ? -1.0 : (hdet > 1.0 ? 1.0 : hdet);
        const double phi = acos(hdet) / 3.0;
        lam = q + 2.0 * p * cos(phi + 2.0943951023931954923);                   // + 2 pi / 3: the smallest of the three roots
    }
    const double m00 = a00 - lam, m11 = a11 - lam, m22 = a22 - lam;
    const double r0[3] = {m00, a01, a02}, r1[3] = {a01, m11, a12}, r2[3] = {a02, a12, m22};
    const double x01[3] = {r0[1] * r1[2] - r0[2] * r1[1], r0[2] * r1[0] - r0[0] * r1[2], r0[0] * r1[1] - r0[1] * r1[0]};
    const double x02[3] = {r0[1] * r2[2] - r0[2] * r2[1], r0[2] * r2[0] - r0[0] * r2[2], r0[0] * r2[1] - r0[1] * r2[0]};
    const double x12[3] = {r1[1] * r2[2] - r1[2] * r2[1], r1[2] * r2[0] - r1[0] * r2[2], r1[0] * r2[1] - r1[1] * r2[0]};
    const double d01 = x01[0] * x01[0] + x01[1] * x01[1] + x01[2] * x01[2];
    const double d02 = x02[0] * x02[0] + x02[1] * x02[1] + x02[2] * x02[2];
    const double d12 = x12[0] * x12[0] + x12[1] * x12[1] + x12[2] * x12[2];
    double v0 = x01[0], v1 = x01[1], v2 = x01[2], dm = d01;
    if (d02 > dm) v0 = x02[0], v1 = x02[1], v2 = x02[2], dm = d02;
    if (d12 > dm) v0 = x12[0], v1 = x12[1], v2 = x12[2], dm = d12;
    if (!(dm > 1e-14)) {                                                       // far above what the cubic's root error (~1e-8 at a double root) leaves
        const double n0 = r0[0] * r0[0] + r0[1] * r0[1] + r0[2] * r0[2], n1 = r1[0] * r1[0] + r1[1] * r1[1] + r1[2] * r1[2];
        const double n2 = r2[0] * r2[0] + r2[1] * r2[1] + r2[2] * r2[2];
        double u0 = r0[0], u1 = r0[1], u2 = r0[2], um = n0;
        if (n1 > um) u0 = r1[0], u1 = r1[1], u2 = r1[2], um = n1;
        if (n2 > um) u0 = r2[0], u1 = r2[1], u2 = r2[2], um = n2;
        if (!(um > 0.0)) return;
        const double ax = fabs(u0), ay = fabs(u1), az = fabs(u2);
        if (ax <= ay && ax <= az) v0 = 0.0, v1 = -u2, v2 = u1;                 // e_x x u
        else if (ay <= az) v0 = u2, v1 = 0.0, v2 = -u0;                        // e_y x u
        else v0 = -u1, v1 = u0, v2 = 0.0;                                      // e_z x u
        dm = v0 * v0 + v1 * v1 + v2 * v2;
        if (!(dm > 0.0)) return;
    }
    const double len = sqrt(dm);
    n[0] = v0 / len, n[1] = v1 / len, n[2] = v2 / len;
}

// one thread per point: mean and centred covariance of the kk neighbours in rank order, the eigenvector, the orientation, one fp32 store
__global__ __launch_bounds__(256) void pc_normals_kernel(const float* __restrict__ points, const int* __restrict__ idx, int N, int kk,
                                                         double camx, double camy, double camz, float* __restrict__ normals) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    double n[3] = {0.0, 0.0, 1.0};
    if (kk >= 3) {
        const int* row = idx + (long)i * kk;
        double sx = 0.0, sy = 0.0, sz = 0.0;
        for (int r = 0; r < kk; ++r) {
            const unsigned j = (unsigned)row[r];
            if (j >= (unsigned)N) continue;
            sx = sx + (double)points[3 * (long)j], sy = sy + (double)points[3 * (long)j + 1], sz = sz + (double)points[3 * (long)j + 2];
        }
        const double mx = sx / (double)kk, my = sy / (double)kk, mz = sz / (double)kk;
        double c00 = 0.0, c01 = 0.0, c02 = 0.0, c11 = 0.0, c12 = 0.0, c22 = 0.0;
        for (int r = 0; r < kk; ++r) {
            const unsigned j = (unsigned)row[r];
            if (j >= (unsigned)N) continue;
            const double dx = (double)points[3 * (long)j] - mx, dy = (double)points[3 * (long)j + 1] - my, dz = (double)points[3 * (long)j + 2] - mz;
            c00 = c00 + dx * dx, c01 = c01 + dx * dy, c02 = c02 + dx * dz, c11 = c11 + dy * dy, c12 = c12 + dy * dz, c22 = c22 + dz * dz;
        }
        const double k = (double)kk;
        pc_min_eigenvector(c00 / k, c01 / k, c02 / k, c11 / k, c12 / k, c22 / k, n);
    }
    const double vx = camx - (double)points[3 * (long)i], vy = camy - (double)points[3 * (long)i + 1], vz = camz - (double)points[3 * (long)i + 2];
    if ((n[0] * vx + n[1] * vy) + n[2] * vz < 0.0) n[0] = -n[0], n[1] = -n[1], n[2] = -n[2];
    normals[3 * (long)i] = (float)n[0], normals[3 * (long)i + 1] = (float)n[1], normals[3 * (long)i + 2] = (float)n[2];
}

// one thread per point: the standalone orientation of given normals, with the zero-normal rule
__global__ __launch_bounds__(256) void pc_orient_kernel(const float* __restrict__ points, const float* __restrict__ normals, int N, double camx,
                                                        double camy, double camz, float* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    double nx = (double)normals[3 * (long)i], ny = (double)normals[3 * (long)i + 1], nz = (double)normals[3 * (long)i + 2];
    const double vx = camx - (double)points[3 * (long)i], vy = camy - (double)points[3 * (long)i + 1], vz = camz - (double)points[3 * (long)i + 2];
    if (nx == 0.0 && ny == 0.0 && nz == 0.0) {
        const double len = sqrt((vx * vx + vy * vy) + vz * vz);
        if (len == 0.0) nx = 0.0, ny = 0.0, nz = 1.0;
        else nx = vx / len, ny = vy / len, nz = vz / len;
    } else if ((nx * vx + ny * vy) + nz * vz < 0.0) {
        nx = -nx, ny = -ny, nz = -nz;
    }
    out[3 * (long)i] = (float)nx, out[3 * (long)i + 1] = (float)ny, out[3 * (long)i + 2] = (float)nz;
}

// the grid of an entry point, or false with the error set
bool pc_grid(const char* who, float x0, float y0, float z0, double cell, int gx, int gy, int gz, PcGrid* gr) {
    if (!(cell > 0.0 && cell < 1e300)) {
        orv_set_error("%s: the cell edge must be positive and finite (got %g)", who, cell);
        return false;
    }
    if (!(x0 == x0 && y0 == y0 && z0 == z0 && fabsf(x0) < INFINITY && fabsf(y0) < INFINITY && fabsf(z0) < INFINITY)) {
        orv_set_error("%s: the grid origin must be finite (got %g, %g, %g)", who, x0, y0, z0);
        return false;
    }
    if (!(gx >= 1 && gy >= 1 && gz >= 1 && (long)gx * gy * gz <= PC_MAX_CELLS && (long)gx * gy <= PC_MAX_CELLS)) {
        orv_set_error("%s: the grid is %d x %d x %d cells; supported: at least 1 per axis and at most %ld in all", who, gx, gy, gz, PC_MAX_CELLS);
        return false;
    }
    gr->lo[0] = x0, gr->lo[1] = y0, gr->lo[2] = z0, gr->h = cell, gr->g[0] = gx, gr->g[1] = gy, gr->g[2] = gz;
    return true;
}

}  // namespace

#define PC_REQUIRE_K(who) ORV_REQUIRE(k >= 1 && k <= PC_KMAX, "%s: k = %d neighbours; supported: 1 to %d", who, k, PC_KMAX)
#define PC_MAX_N 0x2aaaaaaa          /* 3 N fits an int on the Python side's buffers and (long) arithmetic everywhere here */

extern "C" int orv_pc_cells(const float* points, int N, float x0, float y0, float z0, double cell, int gx, int gy, int gz, long* keys,
                            void* stream) {
    const char* who = "orv_pc_cells";
    ORV_REQUIRE(N >= 0 && N <= PC_MAX_N, "%s: N must not be negative or above %d (got %d)", who, PC_MAX_N, N);
    PcGrid gr;
    if (!pc_grid(who, x0, y0, z0, cell, gx, gy, gz, &gr)) return ORV_EINVAL;
    if (N == 0) return ORV_OK;
    ORV_REQUIRE(points && keys, "%s: null pointer (points / keys)", who);
    ORV_REQUIRE(orv_aligned(points, 4) && orv_aligned(keys, 8), "%s: points must be 4-byte and keys 8-byte aligned", who);
    hipLaunchKernelGGL(pc_cells_kernel, dim3(orv_blocks(N, 256)), dim3(256), 0, (hipStream_t)stream, points, N, gr, keys);
    return orv_check_launch(who);
}

extern "C" int orv_pc_cell_table(const long* sorted_keys, const long* order, const float* points, int N, int n_cells, int* start,
                                 float* sorted_points, void* stream) {
    const char* who = "orv_pc_cell_table";
    ORV_REQUIRE(N >= 0 && N <= PC_MAX_N, "%s: N must not be negative or above %d (got %d)", who, PC_MAX_N, N);
    ORV_REQUIRE(n_cells >= 1 && n_cells <= PC_MAX_CELLS, "%s: n_cells = %d; supported: 1 to %ld", who, n_cells, PC_MAX_CELLS);
    if (N == 0) return ORV_OK;
    ORV_REQUIRE(sorted_keys && order && points && start && sorted_points, "%s: null pointer", who);
    ORV_REQUIRE(orv_aligned(sorted_keys, 8) && orv_aligned(order, 8) && orv_aligned(points, 4) && orv_aligned(start, 4) && orv_aligned(sorted_points, 4),
                "%s: sorted_keys and order must be 8-byte, points, start and sorted_points 4-byte aligned", who);
    const long threads = N > n_cells + 1 ? N : n_cells + 1;
    hipLaunchKernelGGL(pc_cell_table_kernel, dim3(orv_blocks(threads, 256)), dim3(256), 0, (hipStream_t)stream, sorted_keys, order, points, N, n_cells,
                       start, sorted_points);
    return orv_check_launch(who);
}

extern "C" int orv_pc_knn(const float* sorted_points, const long* order, const int* start, int N, int k, float x0, float y0, float z0,
                          double cell, int gx, int gy, int gz, int* idx, double* d2, unsigned char* pending, void* stream) {
    const char* who = "orv_pc_knn";
    ORV_REQUIRE(N >= 0 && N <= PC_MAX_N, "%s: N must not be negative or above %d (got %d)", who, PC_MAX_N, N);
    PC_REQUIRE_K(who);
    PcKnnArgs a;
    if (!pc_grid(who, x0, y0, z0, cell, gx, gy, gz, &a.gr)) return ORV_EINVAL;
    if (N == 0) return ORV_OK;
    ORV_REQUIRE(sorted_points && order && start, "%s: null pointer (sorted_points / order / start)", who);
    ORV_REQUIRE(idx && d2 && pending, "%s: null pointer (idx / d2 / pending)", who);
    ORV_REQUIRE(orv_aligned(order, 8) && orv_aligned(d2, 8) && orv_aligned(sorted_points, 4) && orv_aligned(start, 4) && orv_aligned(idx, 4),
                "%s: order and d2 must be 8-byte, sorted_points, start and idx 4-byte aligned", who);
    a.sorted_points = sorted_points, a.order = order, a.start = start, a.idx = idx, a.d2 = d2, a.pending = pending;
    a.N = N, a.kk = k < N ? k : N;
    hipLaunchKernelGGL(pc_knn_kernel, dim3(orv_blocks(N, 4)), dim3(256), 0, (hipStream_t)stream, a);
    return orv_check_launch(who);
}

extern "C" int orv_pc_knn_brute(const float* points, int N, int k, const long* queries, int Q, int* idx, double* d2, void* stream) {
    const char* who = "orv_pc_knn_brute";
    ORV_REQUIRE(N >= 0 && N <= PC_MAX_N, "%s: N must not be negative or above %d (got %d)", who, PC_MAX_N, N);
    PC_REQUIRE_K(who);
    ORV_REQUIRE(Q >= 0 && Q <= N, "%s: Q = %d queries must be in [0, N = %d]", who, Q, N);
    if (N == 0 || Q == 0) return ORV_OK;
    ORV_REQUIRE(points && queries && idx && d2, "%s: null pointer (points / queries / idx / d2)", who);
    ORV_REQUIRE(orv_aligned(queries, 8) && orv_aligned(d2, 8) && orv_aligned(points, 4) && orv_aligned(idx, 4),
                "%s: queries and d2 must be 8-byte, points and idx 4-byte aligned", who);
    hipLaunchKernelGGL(pc_knn_brute_kernel, dim3((unsigned)Q), dim3(256), 0, (hipStream_t)stream, points, N, k < N ? k : N, queries, idx, d2);
    return orv_check_launch(who);
}

extern "C" long orv_pc_outlier_workspace(int N) {
    if (N <= 0) return 0;
    return 2L * (long)orv_blocks(N, PC_CHUNK) * (long)sizeof(double);
}

extern "C" int orv_pc_outlier(const double* d2, int N, int k, double std_ratio, double* avg, double* stats, unsigned char* keep,
                              void* workspace, long workspace_bytes, void* stream) {
    const char* who = "orv_pc_outlier";
    ORV_REQUIRE(N >= 0 && N <= PC_MAX_N, "%s: N must not be negative or above %d (got %d)", who, PC_MAX_N, N);
    PC_REQUIRE_K(who);
    ORV_REQUIRE(std_ratio == std_ratio && fabs(std_ratio) < 1e300, "%s: std_ratio must be finite (got %g)", who, std_ratio);
    ORV_REQUIRE(stats, "%s: null pointer (stats)", who);
    if (N == 0) return ORV_OK;
    ORV_REQUIRE(d2 && avg && keep && workspace, "%s: null pointer (d2 / avg / keep / workspace)", who);
    ORV_REQUIRE(orv_aligned(d2, 8) && orv_aligned(avg, 8) && orv_aligned(stats, 8) && orv_aligned(workspace, 8),
                "%s: d2, avg, stats and workspace must be 8-byte aligned", who);
    const long need = orv_pc_outlier_workspace(N);
    ORV_REQUIRE(workspace_bytes >= need, "%s: the workspace holds %ld bytes; orv_pc_outlier_workspace(%d) = %ld", who, workspace_bytes, N, need);
    hipStream_t s = (hipStream_t)stream;
    const int kk = k < N ? k : N, nb = (int)orv_blocks(N, PC_CHUNK);
    double* partials = (double*)workspace;
    hipLaunchKernelGGL(pc_avg_kernel, dim3(orv_blocks(N, 256)), dim3(256), 0, s, d2, N, kk, avg);
    hipLaunchKernelGGL(pc_partial_kernel, dim3((unsigned)nb), dim3(256), 0, s, (const double*)avg, N, (const double*)nullptr, partials);
    hipLaunchKernelGGL(pc_final_kernel, dim3(1), dim3(256), 0, s, (const double*)partials, nb, 0, std_ratio, stats);
    hipLaunchKernelGGL(pc_partial_kernel, dim3((unsigned)nb), dim3(256), 0, s, (const double*)avg, N, (const double*)stats, partials);
    hipLaunchKernelGGL(pc_final_kernel, dim3(1), dim3(256), 0, s, (const double*)partials, nb, 1, std_ratio, stats);
    hipLaunchKernelGGL(pc_mask_kernel, dim3(orv_blocks(N, 256)), dim3(256), 0, s, (const double*)avg, N, (const double*)stats, keep);
    return orv_check_launch(who);
}

extern "C" int orv_pc_normals(const float* points, const int* idx, int N, int k, double camx, double camy, double camz, float* normals,
                              void* stream) {
    const char* who = "orv_pc_normals";
    ORV_REQUIRE(N >= 0 && N <= PC_MAX_N, "%s: N must not be negative or above %d (got %d)", who, PC_MAX_N, N);
    PC_REQUIRE_K(who);
    ORV_REQUIRE(camx == camx && camy == camy && camz == camz && fabs(camx) < 1e300 && fabs(camy) < 1e300 && fabs(camz) < 1e300,
                "%s: the camera location must be finite (got %g, %g, %g)", who, camx, camy, camz);
    if (N == 0) return ORV_OK;
    ORV_REQUIRE(points && idx && normals, "%s: null pointer (points / idx / normals)", who);
    ORV_REQUIRE(orv_aligned(points, 4) && orv_aligned(idx, 4) && orv_aligned(normals, 4), "%s: points, idx and normals must be 4-byte aligned", who);
    hipLaunchKernelGGL(pc_normals_kernel, dim3(orv_blocks(N, 256)), dim3(256), 0, (hipStream_t)stream, points, idx, N, k < N ? k : N, camx, camy, camz,
                       normals);
    return orv_check_launch(who);
}

extern "C" int orv_pc_orient(const float* points, const float* normals, int N, double camx, double camy, double camz, float* out, void* stream) {
    const char* who = "orv_pc_orient";
    ORV_REQUIRE(N >= 0 && N <= PC_MAX_N, "%s: N must not be negative or above %d (got %d)", who, PC_MAX_N, N);
    ORV_REQUIRE(camx == camx && camy == camy && camz == camz && fabs(camx) < 1e300 && fabs(camy) < 1e300 && fabs(camz) < 1e300,
                "%s: the camera location must be finite (got %g, %g, %g)", who, camx, camy, camz);
    if (N == 0) return ORV_OK;
    ORV_REQUIRE(points && normals && out, "%s: null pointer (points / normals / out)", who);
    ORV_REQUIRE(orv_aligned(points, 4) && orv_aligned(normals, 4) && orv_aligned(out, 4), "%s: points, normals and out must be 4-byte aligned", who);
    hipLaunchKernelGGL(pc_orient_kernel, dim3(orv_blocks(N, 256)), dim3(256), 0, (hipStream_t)stream, points, normals, N, camx, camy, camz, out);
    return orv_check_launch(who);
}
