// Device-side snapshot of a training state with a checksum per tensor (orv_amd.train_state).
//
// A table of n entries {src, dst, bytes} is copied src -> dst in ONE launch and every entry gets the pair (s1, s2) of the checksum
// contract, written by a second, fixed combine launch.  An entry whose dst is NULL is summed only (orv_checksum: every entry).
//
//   The contract (integer arithmetic, every operation mod 2^64): the entry's bytes, padded with zero bytes to a multiple of 4, read as
//   little-endian u32 words w_0 .. w_{W-1};  s1 = sum w_i;  s2 = sum (i + 1) w_i.  An empty entry gives (0, 0).
//
// Geometry: an entry is cut into chunks of SNAP_CHUNK bytes of ITS OWN byte range (the last one shorter); the chunks of the whole table,
// in table order, are dealt round-robin to a grid of at most SNAP_GRID workgroups.  A workgroup finds the entry of its next chunk by
// walking the table forward from where its last chunk was (chunk numbers only grow, so it reads the table once in its life).  Per chunk c
// of an entry, with first word index base_c = c * SNAP_CHUNK / 4, the workgroup keeps s1_c = sum w and t_c = sum (j + 1) w over the
// chunk's own word numbers j and stores the pair (s1_c, t_c + base_c * s1_c) at the chunk's slot of `scratch`; the combine launch adds an
// entry's slots.  Both sums are modular, so the result does not depend on the order - and still no atomics: fixed slots, fixed second pass.
//
// Inside a chunk: dst (src when only summing) fixes the alignment.  Up to three leading words bring it to 16 bytes, the body moves as
// 16-byte accesses (the store aligned; the load is 16 bytes wide at src's own 4-byte alignment), up to three words follow, and the last
// 1-3 bytes of an entry travel as bytes - zero-padded in the sum only, nothing is written past dst + bytes.  Plain vector stores.
#include "common.hpp"

namespace {

constexpr int SNAP_CHUNK = 16384;               // bytes per chunk: 256 lanes x 4 accesses of 16 bytes
constexpr int SNAP_WORDS = SNAP_CHUNK / 4;
constexpr int SNAP_GRID = 2048;                 // 256 CUs x 8 workgroups
constexpr int SNAP_MAX_ENTRIES = 1 << 20;

typedef unsigned long long u64;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 u32x4_a4 __attribute__((aligned(4)));          // a 16-byte access at 4-byte alignment
// the table's pointers are device memory: say so, or every access is a flat one
#define SNAP_GLOBAL __attribute__((address_space(1)))

__device__ __forceinline__ long snap_chunks(long bytes) { return (bytes + SNAP_CHUNK - 1) / SNAP_CHUNK; }

// sum of (a, b) over the 256 lanes of the workgroup, valid in thread 0; `red` is 8 u64 of LDS, reusable after the next barrier
__device__ __forceinline__ void block_sum2(u64& a, u64& b, u64* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o, 64);
        b += __shfl_xor(b, o, 64);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[2 * wave] = a; red[2 * wave + 1] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        a = red[0] + red[2] + red[4] + red[6];
        b = red[1] + red[3] + red[5] + red[7];
    }
}

__global__ __launch_bounds__(256) void snapshot_kernel(const orv_snapshot_entry_t* __restrict__ entries, int n, long total_chunks,
                                                       u64* __restrict__ partials) {
    __shared__ u64 red[8];
    const int t = threadIdx.x;
    int e = 0;
    long first = 0;                 // number of the first chunk of entry e
    for (long g = blockIdx.x; g < total_chunks; g += gridDim.x) {
        // uniform walk: the entry that holds chunk g (the host counted total_chunks from the same table, so e stays below n; the bound
        // keeps a table that changed in between from running off its end)
        long have = snap_chunks(entries[e].bytes);
        while (g >= first + have && e + 1 < n) {
            first += have;
            ++e;
            have = snap_chunks(entries[e].bytes);
        }
        const long c = g - first;
        u64 s1 = 0, tt = 0;
        if (c < have) {
            const long bytes = entries[e].bytes;
            const long off = c * SNAP_CHUNK;
            const int len = (int)(bytes - off < SNAP_CHUNK ? bytes - off : SNAP_CHUNK);
            const SNAP_GLOBAL unsigned char* src = (const SNAP_GLOBAL unsigned char*)entries[e].src + off;
            SNAP_GLOBAL unsigned char* dst = entries[e].dst ? (SNAP_GLOBAL unsigned char*)entries[e].dst + off : nullptr;
            const SNAP_GLOBAL uint32_t* s32 = (const SNAP_GLOBAL uint32_t*)src;
            SNAP_GLOBAL uint32_t* d32 = (SNAP_GLOBAL uint32_t*)dst;
            const int full = len >> 2, rem = len & 3;
            const int lead = (int)((0 - (uintptr_t)(dst ? dst : src)) & 15) >> 2;
            const int head = lead < full ? lead : full;
            const int nvec = (full - head) >> 2;
            const int post = full - head - 4 * nvec;
            // body: 16 bytes per lane and access, every load issued before the first store
            u32x4 r[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int v = t + 256 * k;
                if (v < nvec) r[k] = *(const SNAP_GLOBAL u32x4_a4*)(s32 + head + 4 * v);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int v = t + 256 * k;
                if (v < nvec) {
                    if (d32) *(SNAP_GLOBAL u32x4*)(d32 + head + 4 * v) = r[k];
                    const uint32_t j = (uint32_t)(head + 4 * v) + 1u;         // word number + 1, at most SNAP_WORDS
                    s1 += (u64)r[k].x + r[k].y + r[k].z + r[k].w;
                    tt += (u64)j * r[k].x + (u64)(j + 1) * r[k].y + (u64)(j + 2) * r[k].z + (u64)(j + 3) * r[k].w;
                }
            }
            // the words in front of and behind the body (at most three each), one lane per word
            if (t < head + post) {
                const int j = t < head ? t : head + 4 * nvec + (t - head);
                const uint32_t w = s32[j];
                if (d32) d32[j] = w;
                s1 += w;
                tt += (u64)(uint32_t)(j + 1) * w;
            }
            // the last 1-3 bytes of the entry: copied as bytes, summed as one zero-padded word
            if (t == 8 && rem) {
                uint32_t w = 0;
                for (int b = 0; b < rem; ++b) {
                    const unsigned char x = src[4 * full + b];
                    if (dst) dst[4 * full + b] = x;
                    w |= (uint32_t)x << (8 * b);
                }
                s1 += w;
                tt += (u64)(uint32_t)(full + 1) * w;
            }
        }
        block_sum2(s1, tt, red);
        if (t == 0) {
            const u64 base = (u64)c * SNAP_WORDS;
            *(ulonglong2*)(partials + 2 * g) = make_ulonglong2(s1, tt + base * s1);
        }
        __syncthreads();            // `red` is free again
    }
}

// one workgroup per entry: its first chunk number (the chunk counts of the entries before it), then the sum of its chunks' pairs
__global__ __launch_bounds__(256) void snapshot_combine_kernel(const orv_snapshot_entry_t* __restrict__ entries, long total_chunks,
                                                               const u64* __restrict__ partials, u64* __restrict__ sums) {
    __shared__ u64 red[8];
    __shared__ u64 first_s;
    const int e = blockIdx.x, t = threadIdx.x;
    u64 first = 0, unused = 0;
    for (int i = t; i < e; i += 256) first += (u64)snap_chunks(entries[i].bytes);
    block_sum2(first, unused, red);
    if (t == 0) first_s = first;
    __syncthreads();
    const long lo = (long)first_s;
    long hi = lo + snap_chunks(entries[e].bytes);
    if (hi > total_chunks) hi = total_chunks;
    u64 s1 = 0, s2 = 0;
    for (long g = lo + t; g < hi; g += 256) {
        const ulonglong2 p = *(const ulonglong2*)(partials + 2 * g);
        s1 += p.x;
        s2 += p.y;
    }
    block_sum2(s1, s2, red);
    if (t == 0) *(ulonglong2*)(sums + 2 * (long)e) = make_ulonglong2(s1, s2);
}

// Everything that can be checked without following a device pointer; -> number of chunks, or -1 with the error set.
long snap_validate(const char* who, const orv_snapshot_entry_t* entries, const orv_snapshot_entry_t* host, int n, const void* sums,
                   const void* scratch, long scratch_bytes, bool sum_only) {
    if (!entries || !host) {
        orv_set_error("%s: null table (entries is the device table, entries_host the same n entries in host memory)", who);
        return -1;
    }
    if (n < 1 || n > SNAP_MAX_ENTRIES) { orv_set_error("%s: n=%d entries (supported: 1 .. %d)", who, n, SNAP_MAX_ENTRIES); return -1; }
    if (!sums || !orv_aligned(sums, 16)) { orv_set_error("%s: sums (u64 [n][2]) must be a 16-byte aligned device buffer", who); return -1; }
    long chunks = 0;
    for (int i = 0; i < n; ++i) {
        const orv_snapshot_entry_t& x = host[i];
        if (x.bytes < 0) { orv_set_error("%s: entry %d has bytes=%ld", who, i, x.bytes); return -1; }
        if (!x.src && x.bytes > 0) { orv_set_error("%s: entry %d has a null src with bytes=%ld", who, i, x.bytes); return -1; }
        if (!orv_aligned(x.src, 4) || !orv_aligned(x.dst, 4)) {
            orv_set_error("%s: entry %d: src and dst must be 4-byte aligned (any residue 0 / 4 / 8 / 12 mod 16 is taken)", who, i);
            return -1;
        }
        if (sum_only && x.dst) { orv_set_error("%s: entry %d has a dst; the checksum writes nothing (dst must be NULL)", who, i); return -1; }
        if (x.dst && (uintptr_t)x.src < (uintptr_t)x.dst + (uintptr_t)x.bytes && (uintptr_t)x.dst < (uintptr_t)x.src + (uintptr_t)x.bytes) {
            orv_set_error("%s: entry %d: src and dst overlap", who, i);
            return -1;
        }
        chunks += (x.bytes + SNAP_CHUNK - 1) / SNAP_CHUNK;
        if (chunks > 0x7fffffffL) { orv_set_error("%s: more than 2^31 chunks of %d bytes", who, SNAP_CHUNK); return -1; }
    }
    if (chunks > 0 && (!scratch || !orv_aligned(scratch, 16) || scratch_bytes < 16 * chunks)) {
        orv_set_error("%s: scratch must be a 16-byte aligned device buffer of at least %ld bytes for this table (got %ld; "
                      "orv_snapshot_scratch_bytes bounds it)", who, 16 * chunks, scratch_bytes);
        return -1;
    }
    return chunks;
}

int snap_launch(const char* who, const orv_snapshot_entry_t* entries, int n, long chunks, void* sums, void* scratch, void* stream) {
    if (chunks > 0) {
        const unsigned grid = (unsigned)(chunks < SNAP_GRID ? chunks : SNAP_GRID);
        hipLaunchKernelGGL(snapshot_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, entries, n, chunks, (u64*)scratch);
    }
    hipLaunchKernelGGL(snapshot_combine_kernel, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, entries, chunks, (const u64*)scratch,
                       (u64*)sums);
    return orv_check_launch(who);
}

}  // namespace

extern "C" int orv_snapshot_chunk_bytes(void) { return SNAP_CHUNK; }

extern "C" long orv_snapshot_scratch_bytes(int n, long total_bytes) {
    if (n < 1 || n > SNAP_MAX_ENTRIES || total_bytes < 0) {
        orv_set_error("orv_snapshot_scratch_bytes: n=%d entries (supported: 1 .. %d), total_bytes=%ld (supported: >= 0)", n, SNAP_MAX_ENTRIES,
                      total_bytes);
        return -1;
    }
    return 16 * (total_bytes / SNAP_CHUNK + n);          // at most one partly filled chunk per entry
}

extern "C" int orv_snapshot(const orv_snapshot_entry_t* entries, const orv_snapshot_entry_t* entries_host, int n, unsigned long long* sums,
                            void* scratch, long scratch_bytes, void* stream) {
    const long chunks = snap_validate("orv_snapshot", entries, entries_host, n, sums, scratch, scratch_bytes, false);
    if (chunks < 0) return ORV_EINVAL;
    return snap_launch("orv_snapshot", entries, n, chunks, sums, scratch, stream);
}

extern "C" int orv_checksum(const orv_snapshot_entry_t* entries, const orv_snapshot_entry_t* entries_host, int n, unsigned long long* sums,
                            void* scratch, long scratch_bytes, void* stream) {
    const long chunks = snap_validate("orv_checksum", entries, entries_host, n, sums, scratch, scratch_bytes, true);
    if (chunks < 0) return ORV_EINVAL;
    return snap_launch("orv_checksum", entries, n, chunks, sums, scratch, stream);
}
