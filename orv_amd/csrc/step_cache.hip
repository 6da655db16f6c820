// The first-block step cache of the denoise loop (orv_amd/step_cache.py): three streaming kernels over the video rows of the joint
// [B, S, D] buffer and a small finishing launch.  Written from the contract in DESIGN.md section 20.
//   * probe:  F = the video rows after iteration 0 (dense copy), c = bf16(F - E), and per clip num = sum |c - p|, den = sum |p|.
//   * store:  t = bf16(X - F) from the video rows after the last iteration, and p <- c.
//   * apply:  the video rows become bf16(F + t), in place.
// With ldx = D the video rows of one clip are ONE contiguous range of Nv * D values that starts at row b * S + Nt, so every kernel walks
// 16-byte units (8 bf16) of a range and needs no row arithmetic.  A workgroup of 256 lanes owns SC_TILE = 1024 consecutive units of one clip,
// a lane the units lane, lane + 256, lane + 512, lane + 768 of them: every load of a wave covers 1 KiB of consecutive bytes.
// The sums: each difference is one fp32 subtraction, its absolute value is widened to fp64 and added in fp64 - per lane in unit order, then
// a butterfly over the wave, then the four waves in order, then (finishing launch, one wave per clip) the workgroups' partial sums in a
// strided order and one more butterfly.  The order depends on (Nv, D) only, there are no atomics: two runs give the same bits.
#include "common.hpp"

namespace {

constexpr int SC_LANES = 256;
constexpr int SC_ITEMS = 4;
constexpr int SC_TILE = SC_LANES * SC_ITEMS;      // 16-byte units per workgroup
constexpr int SC_MAX_B = 65535;                   // clips ride on gridDim.y

__device__ __forceinline__ void sc_unpack(const uint4& u, float* v) {
    const unsigned w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) v[2 * k] = __uint_as_float(w[k] << 16), v[2 * k + 1] = __uint_as_float(w[k] & 0xffff0000u);
}
__device__ __forceinline__ uint4 sc_pack(const float* v) {
    unsigned w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) w[k] = (unsigned)f2bf(v[2 * k]) | (unsigned)f2bf(v[2 * k + 1]) << 16;
    return make_uint4(w[0], w[1], w[2], w[3]);
}
__device__ __forceinline__ double sc_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// x: the joint buffer in 16-byte units; clip b's video rows start at unit (b * S + Nt) * (D / 8).  units = Nv * D / 8 per clip.
__global__ __launch_bounds__(SC_LANES) void step_cache_probe_kernel(const uint4* __restrict__ x, long clip_stride, long video_off,
                                                                    const uint4* __restrict__ e, const uint4* __restrict__ p,
                                                                    uint4* __restrict__ f, uint4* __restrict__ c, long units,
                                                                    double* __restrict__ partial) {
    const int b = blockIdx.y;
    const long u0 = (long)blockIdx.x * SC_TILE + threadIdx.x;
    const uint4* xb = x + b * clip_stride + video_off;
    const long d0 = b * units;
    uint4 xv[SC_ITEMS], ev[SC_ITEMS], pv[SC_ITEMS];
#pragma unroll
    for (int k = 0; k < SC_ITEMS; ++k) {
        const long u = u0 + k * SC_LANES;
        if (u < units) xv[k] = xb[u], ev[k] = e[d0 + u], pv[k] = p[d0 + u];
    }
    double num = 0.0, den = 0.0;
#pragma unroll
    for (int k = 0; k < SC_ITEMS; ++k) {
        const long u = u0 + k * SC_LANES;
        if (u < units) {
            float fx[8], fe[8], fp[8], fc[8];
            sc_unpack(xv[k], fx), sc_unpack(ev[k], fe), sc_unpack(pv[k], fp);
#pragma unroll
            for (int i = 0; i < 8; ++i) fc[i] = fx[i] - fe[i];
            const uint4 cv = sc_pack(fc);
            f[d0 + u] = xv[k];
            c[d0 + u] = cv;
            sc_unpack(cv, fc);                                    // the ROUNDED residual enters the distance
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                num += (double)fabsf(fc[i] - fp[i]);
                den += (double)fabsf(fp[i]);
            }
        }
    }
    num = sc_wave_sum(num), den = sc_wave_sum(den);
    __shared__ double red[2][SC_LANES / 64];
    if ((threadIdx.x & 63) == 0) red[0][threadIdx.x >> 6] = num, red[1][threadIdx.x >> 6] = den;
    __syncthreads();
    if (threadIdx.x == 0) {
        double n = red[0][0], d = red[1][0];
#pragma unroll
        for (int w = 1; w < SC_LANES / 64; ++w) n += red[0][w], d += red[1][w];
        double* o = partial + ((long)b * gridDim.x + blockIdx.x) * 2;
        o[0] = n, o[1] = d;
    }
}

// one wave per clip: partial [B, tiles, 2] -> sums [B, 2]
__global__ __launch_bounds__(64) void step_cache_finish_kernel(const double* __restrict__ partial, int tiles, double* __restrict__ sums) {
    const int b = blockIdx.x;
    const double* pb = partial + (long)b * tiles * 2;
    double num = 0.0, den = 0.0;
    for (int i = threadIdx.x; i < tiles; i += 64) num += pb[2 * i], den += pb[2 * i + 1];
    num = sc_wave_sum(num), den = sc_wave_sum(den);
    if (threadIdx.x == 0) sums[2 * b] = num, sums[2 * b + 1] = den;
}

__global__ __launch_bounds__(SC_LANES) void step_cache_store_kernel(const uint4* __restrict__ x, long clip_stride, long video_off,
                                                                    const uint4* __restrict__ f, const uint4* __restrict__ c,
                                                                    uint4* __restrict__ t, uint4* __restrict__ p, long units) {
    const int b = blockIdx.y;
    const long u0 = (long)blockIdx.x * SC_TILE + threadIdx.x;
    const uint4* xb = x + b * clip_stride + video_off;
    const long d0 = b * units;
    uint4 xv[SC_ITEMS], fv[SC_ITEMS], cv[SC_ITEMS];
#pragma unroll
    for (int k = 0; k < SC_ITEMS; ++k) {
        const long u = u0 + k * SC_LANES;
        if (u < units) xv[k] = xb[u], fv[k] = f[d0 + u], cv[k] = c[d0 + u];
    }
#pragma unroll
    for (int k = 0; k < SC_ITEMS; ++k) {
        const long u = u0 + k * SC_LANES;
        if (u < units) {
            float fx[8], ff[8];
            sc_unpack(xv[k], fx), sc_unpack(fv[k], ff);
#pragma unroll
            for (int i = 0; i < 8; ++i) fx[i] = fx[i] - ff[i];
            t[d0 + u] = sc_pack(fx);
            p[d0 + u] = cv[k];
        }
    }
}

__global__ __launch_bounds__(SC_LANES) void step_cache_apply_kernel(uint4* __restrict__ x, long clip_stride, long video_off,
                                                                    const uint4* __restrict__ t, long units) {
    const int b = blockIdx.y;
    const long u0 = (long)blockIdx.x * SC_TILE + threadIdx.x;
    uint4* xb = x + b * clip_stride + video_off;
    const long d0 = b * units;
    uint4 xv[SC_ITEMS], tv[SC_ITEMS];
#pragma unroll
    for (int k = 0; k < SC_ITEMS; ++k) {
        const long u = u0 + k * SC_LANES;
        if (u < units) xv[k] = xb[u], tv[k] = t[d0 + u];
    }
#pragma unroll
    for (int k = 0; k < SC_ITEMS; ++k) {
        const long u = u0 + k * SC_LANES;
        if (u < units) {
            float fx[8], ft[8];
            sc_unpack(xv[k], fx), sc_unpack(tv[k], ft);
#pragma unroll
            for (int i = 0; i < 8; ++i) fx[i] = fx[i] + ft[i];
            xb[u] = sc_pack(fx);
        }
    }
}

struct sc_geom {
    long units, tiles, clip_stride, video_off;
};

// the shape checks all four entry points share; what: the entry point's name for the message
int sc_shape(const char* what, int B, int Nt, int Nv, int D, sc_geom* g) {
    ORV_REQUIRE(B >= 1 && B <= SC_MAX_B, "%s: B = %d; supported: 1 to %d clips", what, B, SC_MAX_B);
    ORV_REQUIRE(Nt >= 0 && Nv >= 1 && (long)Nt + Nv <= 0x7fffffffL, "%s: Nt = %d, Nv = %d; supported: Nt >= 0, Nv >= 1, Nt + Nv < 2^31", what, Nt,
                Nv);
    ORV_REQUIRE(D >= 64 && D % 64 == 0, "%s: D = %d; supported: a positive multiple of 64", what, D);
    g->units = (long)Nv * (D / 8);
    g->tiles = (g->units + SC_TILE - 1) / SC_TILE;
    g->clip_stride = ((long)Nt + Nv) * (D / 8);
    g->video_off = (long)Nt * (D / 8);
    ORV_REQUIRE(g->tiles <= 0x7fffffffL, "%s: a clip of %ld values needs %ld workgroups; supported: at most 2^31 - 1", what, (long)Nv * D, g->tiles);
    return ORV_OK;
}

}  // namespace

extern "C" long orv_step_cache_scratch(int B, int Nv, int D) {
    sc_geom g;
    if (sc_shape("orv_step_cache_scratch", B, 0, Nv, D, &g) != ORV_OK) return -1;
    return 2 * (long)B * g.tiles;
}

extern "C" int orv_step_cache_probe(const void* x, const void* e, const void* p, void* f, void* c, double* scratch, long n_scratch, double* sums,
                                    int B, int Nt, int Nv, int D, void* stream) {
    ORV_REQUIRE(x && e && p && f && c && scratch && sums, "orv_step_cache_probe: null pointer (x / e / p / f / c / scratch / sums)");
    sc_geom g;
    if (int rc = sc_shape("orv_step_cache_probe", B, Nt, Nv, D, &g)) return rc;
    ORV_REQUIRE(orv_aligned(x, 16) && orv_aligned(e, 16) && orv_aligned(p, 16) && orv_aligned(f, 16) && orv_aligned(c, 16),
                "orv_step_cache_probe: x, e, p, f and c must be 16-byte aligned");
    ORV_REQUIRE(orv_aligned(scratch, 8) && orv_aligned(sums, 8), "orv_step_cache_probe: scratch and sums must be 8-byte aligned");
    ORV_REQUIRE(n_scratch >= 2 * (long)B * g.tiles, "orv_step_cache_probe: scratch holds %ld doubles, orv_step_cache_scratch(B, Nv, D) = %ld are needed",
                n_scratch, 2 * (long)B * g.tiles);
    ORV_REQUIRE(f != c && f != p && c != p && f != e && c != e, "orv_step_cache_probe: f and c must not alias each other, e or p");
    hipStream_t st = (hipStream_t)stream;
    step_cache_probe_kernel<<<dim3((unsigned)g.tiles, (unsigned)B), dim3(SC_LANES), 0, st>>>(
        (const uint4*)x, g.clip_stride, g.video_off, (const uint4*)e, (const uint4*)p, (uint4*)f, (uint4*)c, g.units, scratch);
    if (int rc = orv_check_launch("orv_step_cache_probe")) return rc;
    step_cache_finish_kernel<<<dim3((unsigned)B), dim3(64), 0, st>>>(scratch, (int)g.tiles, sums);
    return orv_check_launch("orv_step_cache_probe (finish)");
}

extern "C" int orv_step_cache_store(const void* x, const void* f, const void* c, void* t, void* p, int B, int Nt, int Nv, int D, void* stream) {
    ORV_REQUIRE(x && f && c && t && p, "orv_step_cache_store: null pointer (x / f / c / t / p)");
    sc_geom g;
    if (int rc = sc_shape("orv_step_cache_store", B, Nt, Nv, D, &g)) return rc;
    ORV_REQUIRE(orv_aligned(x, 16) && orv_aligned(f, 16) && orv_aligned(c, 16) && orv_aligned(t, 16) && orv_aligned(p, 16),
                "orv_step_cache_store: x, f, c, t and p must be 16-byte aligned");
    ORV_REQUIRE(t != p && t != f && t != c && p != f && p != c, "orv_step_cache_store: t and p must not alias each other, f or c");
    step_cache_store_kernel<<<dim3((unsigned)g.tiles, (unsigned)B), dim3(SC_LANES), 0, (hipStream_t)stream>>>(
        (const uint4*)x, g.clip_stride, g.video_off, (const uint4*)f, (const uint4*)c, (uint4*)t, (uint4*)p, g.units);
    return orv_check_launch("orv_step_cache_store");
}

extern "C" int orv_step_cache_apply(void* x, const void* t, int B, int Nt, int Nv, int D, void* stream) {
    ORV_REQUIRE(x && t, "orv_step_cache_apply: null pointer (x / t)");
    sc_geom g;
    if (int rc = sc_shape("orv_step_cache_apply", B, Nt, Nv, D, &g)) return rc;
    ORV_REQUIRE(orv_aligned(x, 16) && orv_aligned(t, 16), "orv_step_cache_apply: x and t must be 16-byte aligned");
    ORV_REQUIRE(x != t, "orv_step_cache_apply: x and t must not alias");
    step_cache_apply_kernel<<<dim3((unsigned)g.tiles, (unsigned)B), dim3(SC_LANES), 0, (hipStream_t)stream>>>(
        (uint4*)x, g.clip_stride, g.video_off, (const uint4*)t, g.units);
    return orv_check_launch("orv_step_cache_apply");
}
