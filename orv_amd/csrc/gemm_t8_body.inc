// Body of gemm_t8_kernel<BN, EPI> / gemm_t8r192_kernel<BN, EPI> (gemm_t8.hip includes this file once per kernel, with `constexpr int MB` = 16-row
// blocks per m half of a wave set by the including kernel: 4 = 256-row tiles, 3 = 192-row tiles).  One text for both so that the 256-row kernels
// keep their instruction streams to the byte; the K-tile macros defined here are also what gemm_t8_tn_kernel reuses.
    constexpr int NBW = BN / 64;                      // 16-column blocks per wave
    constexpr int RPH = 16 * MB;                      // rows per m half of a wave
    constexpr int BM = 4 * RPH;                       // tile rows: 2 wave rows x 2 m halves
    constexpr int HALF = 16384;                       // A0 | A1 | B region 0 | B region 1
    constexpr int BUF = BN == 256 ? 65536 : 57344;    // BN = 192: the second B region (block 2 of every wave) is 64 rows = 8 KiB
    constexpr int SCR = 2 * BUF;                      // epilogue transpose scratch: 8 waves x 4 KiB behind the two K-tile buffers
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wr = wave >> 2, wc = wave & 3;
    const int ntiles = p.tiles_m * p.tiles_n;
    const int nk = p.K / BK;                          // even (chooser-checked)

    // ---- DMA side.  One wave instruction fills one 1-KiB piece of LDS; the image is lane-linear (lane l writes physical bytes [16 l, 16 l + 16)),
    // so WHICH 16 global bytes a lane fetches decides the layout.  Two layouts, chosen per instantiation (FL):
    //   st_16x32 (the template's): a piece = 16 rows x 32 k; lane l holds logical byte 16 (l ^ ((l >> 5) << 1)): row = that >> 2, 16-byte k-chunk
    //     = that & 3; the two k halves of a 16-row block are two instructions 64 B apart in memory.
    //   full-line (round 4): a piece = 8 rows x 64 k = 8 whole 128-byte lines (lanes 8 r .. 8 r + 7 fetch row r), so the texture path handles 8
    //     full lines per instruction instead of 16 half lines: the LDS-DMA stream ALONE is 13-18 % faster (profiles/r4_gemm_t8_load_side.txt).
    //     Lane l holds physical chunk l & 7 of row r = l >> 3 and fetches logical chunk (l & 7) ^ (r & 6); with that XOR the 16 lanes of every
    //     ds_read_b128 group (row i of a 16-row block = piece i >> 3, row i & 7; k chunk (4 kh + g) ^ (i & 6)) cover the 16 bank slots once.  A
    //     block's two pieces are two instructions 8 rows apart.  In the model (same box, interleaved): FFN1 0.3008 -> 0.2958 ms, FFN2 0.3030 ->
    //     0.2970, out-projection level, q | k | v 0.2326 -> 0.2350 - hence per epilogue: GELU and gated-residual instantiations only.
    // Both: every instruction has its own 32-bit per-lane byte offset (row clamp to M - 1 included, recomputed per output tile) against a
    // wave-uniform base that carries the K position (global_load_lds saddr form: no vector address arithmetic in the K loop).  Needs
    // M * lda * 2 and N * ldw * 2 < 4 GiB (the chooser checks).
    constexpr bool FL = EPI == 1 || EPI == 2;
    const int lsw = FL ? lane : lane ^ ((lane >> 5) << 1);
    const int srow = FL ? lane >> 3 : lsw >> 2;
    const int schunk = FL ? (lane & 7) ^ (srow & 6) : lsw & 3;
    const int q = wave * 16 + srow;                   // row of a 128-row half-tile this lane feeds with its first instruction (FL: second = + 8)
    const int arow0 = (q / RPH) * (2 * RPH) + (q % RPH);      // + h * RPH: tile row held by row q of A half h (MB = 4: (q >> 6) * 128 + (q & 63))
    const bool a_on = MB == 4 || wave < 2 * MB;       // wave-uniform: this wave's rows 16 w .. 16 w + 15 of an A half exist (2 RPH rows)
    int brow0, brow1;                                 // tile column held by row q of B region 0 / by this lane's row of region 1
    {
        const int wc_ = q >> 5, nb_ = (q >> 4) & 1, r = q & 15;
        if (BN == 256) {
            brow0 = wc_ * 64 + 8 * (r >> 2) + 4 * nb_ + (r & 3);      // FL second instruction (r + 8): + 16
            brow1 = brow0 + 32;
        } else {
            brow0 = wc_ * 48 + 8 * (r >> 2) + 4 * nb_ + (r & 3);
            // region 1: 64 rows.  st_16x32: wave w fills (row block w >> 1, k half w & 1); FL: rows 8 (w & 1) .. + 7 of block w >> 1
            brow1 = (wave >> 1) * 48 + 32 + (FL ? (wave & 1) * 8 : 0) + srow;
        }
    }
    const int koff1 = (BN == 256 || FL) ? schunk * 8 : (wave & 1) * 32 + schunk * 8;
    char* const dst2 = smem + wave * 2048;            // two-instruction streams: + S * BUF + region * HALF (+ 1024: second instruction)
    char* const dst1 = smem + 3 * HALF + wave * 1024; // BN = 192 region 1: + S * BUF
    unsigned oA0[2], oA1[2], oB0[2], oB1[2];          // byte offsets from p.A / p.W of the two instructions of a stream
    int kA0 = 0, kA1 = 0, kB0 = 0, kB1 = 0;
    int tA0 = blockIdx.x, tA1 = blockIdx.x, tB0 = blockIdx.x, tB1 = blockIdx.x;
#define T8_SETUP_A(OFF, H, TILE)                                                                                     \
    {                                                                                                                \
        int tm_, tn_;                                                                                                \
        tile_of_index(p, min((TILE), ntiles - 1), ntiles, tm_, tn_);                                                 \
        if (p.dbg == 77) tm_ = 0;   /* ORV_GEMM_DBG=77 (timing experiment, wrong results): every workgroup streams the panels of tile (0, 0) */ \
        const int row_ = tm_ * BM + arow0 + (H) * RPH;                                                               \
        OFF[0] = (unsigned)(((long)min(row_, p.M - 1) * p.lda + schunk * 8) * 2);                                    \
        OFF[1] = FL ? (unsigned)(((long)min(row_ + 8, p.M - 1) * p.lda + schunk * 8) * 2) : OFF[0] + 64;             \
    }
#define T8_SETUP_B(OFF, H, TILE)                                                                                     \
    {                                                                                                                \
        int tm_, tn_;                                                                                                \
        tile_of_index(p, min((TILE), ntiles - 1), ntiles, tm_, tn_);                                                 \
        if (p.dbg == 77) tn_ = 0;                                                                                    \
        const int row_ = tn_ * BN + ((H) == 0 ? brow0 : brow1);                                                      \
        OFF[0] = (unsigned)(((long)row_ * p.ldw + ((H) == 0 ? schunk * 8 : koff1)) * 2);                             \
        OFF[1] = FL ? (unsigned)(((long)(row_ + 16) * p.ldw + schunk * 8) * 2) : OFF[0] + 64;                        \
    }
    // advance a stream by one K-tile; past its tile's last K-tile it moves to the workgroup's next tile (past the last tile: the
    // final tile again - uniform instruction counts, data never read)
#define T8_NEXT_A(OFF, KC, TC, H)                                                                                    \
    if (__builtin_expect(++KC == nk, 0)) { KC = 0; TC += gridDim.x; T8_SETUP_A(OFF, H, TC) }
#define T8_NEXT_B(OFF, KC, TC, H)                                                                                    \
    if (__builtin_expect(++KC == nk, 0)) { KC = 0; TC += gridDim.x; T8_SETUP_B(OFF, H, TC) }
#define T8_GLDS(BASE, KC, OFF, DST) glds16((const char*)(BASE) + (long)(KC) * (BK * 2) + (OFF), DST)
#define T8_ISSUE_A0(S) { if (a_on) { T8_GLDS(p.A, kA0, oA0[0], dst2 + (S) * BUF); T8_GLDS(p.A, kA0, oA0[1], dst2 + (S) * BUF + 1024); } T8_NEXT_A(oA0, kA0, tA0, 0) }
#define T8_ISSUE_A1(S) { if (a_on) { T8_GLDS(p.A, kA1, oA1[0], dst2 + (S) * BUF + HALF); T8_GLDS(p.A, kA1, oA1[1], dst2 + (S) * BUF + HALF + 1024); } T8_NEXT_A(oA1, kA1, tA1, 1) }
// counted wait: N = instructions of the newest, still-allowed group of a wave that feeds both operands; a wave without A pieces has only its two
// region-0 W instructions newer than what must have landed
#define T8_VMCNT(N) { if (a_on) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(N) : "memory"); else asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); }
#define T8_ISSUE_B0(S) { T8_GLDS(p.W, kB0, oB0[0], dst2 + (S) * BUF + 2 * HALF); T8_GLDS(p.W, kB0, oB0[1], dst2 + (S) * BUF + 2 * HALF + 1024); T8_NEXT_B(oB0, kB0, tB0, 0) }
#define T8_ISSUE_B1(S)                                                                                               \
    {                                                                                                                \
        if constexpr (BN == 256) { T8_GLDS(p.W, kB1, oB1[0], dst2 + (S) * BUF + 3 * HALF); T8_GLDS(p.W, kB1, oB1[1], dst2 + (S) * BUF + 3 * HALF + 1024); } \
        else { T8_GLDS(p.W, kB1, oB1[0], dst1 + (S) * BUF); }                                                        \
        T8_NEXT_B(oB1, kB1, tB1, 1)                                                                                  \
    }
    T8_SETUP_A(oA0, 0, tA0)
    T8_SETUP_A(oA1, 1, tA1)
    T8_SETUP_B(oB0, 0, tB0)
    T8_SETUP_B(oB1, 1, tB1)

    // ---- fragment reads.  st_16x32: logical byte (l & 15) * 64 + (l >> 4) * 16 of a piece, bit 5 flipped for rows 8-15, k half 1 = + 1024 (an
    // immediate).  FL: row i = l & 15 of a block = piece i >> 3, row i & 7, k chunk (4 kh + g) ^ (i & 6): k half 1 = the same address with
    // bit 6 flipped (a second base register).
    const int fro = FL ? ((lane & 15) >> 3) * 1024 + (lane & 7) * 128 + (((lane >> 4) ^ (lane & 6)) << 4)
                       : ((lane & 15) * 64 + (lane >> 4) * 16) ^ (((lane >> 3) & 1) << 5);
    const int fro1 = FL ? fro ^ 64 : fro + 1024;
    const char* const rdA = smem + (wr * MB) * 2048 + fro;            // + S * BUF + mh * HALF + mb * 2048
    const char* const rdA_1 = smem + (wr * MB) * 2048 + fro1;
    const char* const rdB = smem + 2 * HALF + (wc * 2) * 2048 + fro;  // region 0 (two blocks per wave): + S * BUF + t * 2048
    const char* const rdB_1 = smem + 2 * HALF + (wc * 2) * 2048 + fro1;
    const char* const rdB1 = BN == 256 ? rdB + HALF : smem + 3 * HALF + wc * 2048 + fro;
    const char* const rdB1_1 = BN == 256 ? rdB_1 + HALF : smem + 3 * HALF + wc * 2048 + fro1;
#define T8_KH(P, KH) (FL ? ((KH) ? P##_1 : P) : P + (KH) * 1024)

    f32x4 acc[2][MB][NBW];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < MB; ++b)
#pragma unroll
            for (int c = 0; c < NBW; ++c) acc[a][b][c] = f32x4{0.f, 0.f, 0.f, 0.f};
    bf16x8 fa[2][MB][2], fb[NBW][2];

#define T8_READ_A(MH, S)                                                                                             \
    _Pragma("unroll") for (int mb = 0; mb < MB; ++mb)                                                                 \
        _Pragma("unroll") for (int kh = 0; kh < 2; ++kh)                                                             \
            fa[MH][mb][kh] = *(const bf16x8*)(T8_KH(rdA, kh) + (S) * BUF + (MH) * HALF + mb * 2048);
#define T8_READ_B01(S)                                                                                               \
    _Pragma("unroll") for (int t = 0; t < 2; ++t)                                                                    \
        _Pragma("unroll") for (int kh = 0; kh < 2; ++kh)                                                             \
            fb[t][kh] = *(const bf16x8*)(T8_KH(rdB, kh) + (S) * BUF + t * 2048);
#define T8_READ_B23(S)                                                                                               \
    _Pragma("unroll") for (int t = 0; t < NBW - 2; ++t)                                                              \
        _Pragma("unroll") for (int kh = 0; kh < 2; ++kh)                                                             \
            fb[2 + t][kh] = *(const bf16x8*)(T8_KH(rdB1, kh) + (S) * BUF + t * 2048);
#define T8_MFMA(MH, B0, NBK)                                                                                         \
    _Pragma("unroll") for (int kh = 0; kh < 2; ++kh)                                                                 \
        _Pragma("unroll") for (int mb = 0; mb < MB; ++mb)                                                             \
            _Pragma("unroll") for (int t = 0; t < (NBK); ++t)                                                        \
                acc[MH][mb][(B0) + t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[(B0) + t][kh], fa[MH][mb][kh], acc[MH][mb][(B0) + t], 0, 0, 0);
#define T8_BAR()                                                                                                     \
    __builtin_amdgcn_sched_barrier(0);                                                                               \
    __builtin_amdgcn_s_barrier();                                                                                    \
    __builtin_amdgcn_sched_barrier(0);
#define T8_LGKM0()                                                                                                   \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                               \
    __builtin_amdgcn_sched_barrier(0);
#define T8_PRIO1() __builtin_amdgcn_s_setprio(1);
#define T8_PRIO0() __builtin_amdgcn_s_setprio(0);

#define T8_KTILE_256(S)                                                                                              \
    {                                                                                                                \
        T8_READ_B01(S)                                                                                               \
        __builtin_amdgcn_sched_barrier(0);                                                                           \
        T8_READ_A(0, S)                                                                                              \
        __builtin_amdgcn_sched_barrier(0);                                                                           \
        T8_ISSUE_B1((S) ^ 1)                                                                                         \
        asm volatile("s_waitcnt lgkmcnt(%0)" :: "n"(2 * MB) : "memory");                                                           \
        T8_BAR() T8_LGKM0() T8_PRIO1() T8_MFMA(0, 0, 2) T8_PRIO0() T8_BAR()                                          \
        T8_READ_A(1, S)                                                                                              \
        __builtin_amdgcn_sched_barrier(0);                                                                           \
        T8_ISSUE_B0(S)                                                                                               \
        T8_BAR() T8_LGKM0() T8_PRIO1() T8_MFMA(1, 0, 2) T8_PRIO0() T8_BAR()                                          \
        T8_READ_B23(S)                                                                                               \
        __builtin_amdgcn_sched_barrier(0);                                                                           \
        T8_ISSUE_A0(S)                                                                                               \
        T8_BAR() T8_LGKM0() T8_PRIO1() T8_MFMA(1, 2, 2) T8_PRIO0() T8_BAR()                                          \
        T8_ISSUE_A1(S)                                                                                               \
        T8_VMCNT(6)                                                                                                          \
        T8_BAR() T8_PRIO1() T8_MFMA(0, 2, 2) T8_PRIO0() T8_BAR()                                                     \
    }
    // BN = 192: P1 (m0, n01) | P2 (m0, n2) + (m1, n2) | P3 (m1, n01); streams: region 1 + A1 of the NEXT K-tile in P1, region 0
    // of K-tile + 2 in P2 (its reads were retired by the lgkmcnt(8) before P1's first barrier), A0 of K-tile + 2 in P3
#define T8_KTILE_192(S)                                                                                              \
    {                                                                                                                \
        T8_READ_B01(S)                                                                                               \
        __builtin_amdgcn_sched_barrier(0);                                                                           \
        T8_READ_A(0, S)                                                                                              \
        __builtin_amdgcn_sched_barrier(0);                                                                           \
        T8_ISSUE_B1((S) ^ 1)                                                                                         \
        T8_ISSUE_A1((S) ^ 1)                                                                                         \
        asm volatile("s_waitcnt lgkmcnt(%0)" :: "n"(2 * MB) : "memory");                                                           \
        T8_BAR() T8_LGKM0() T8_PRIO1() T8_MFMA(0, 0, 2) T8_PRIO0() T8_BAR()                                          \
        T8_READ_B23(S)                                                                                               \
        __builtin_amdgcn_sched_barrier(0);                                                                           \
        T8_READ_A(1, S)                                                                                              \
        __builtin_amdgcn_sched_barrier(0);                                                                           \
        T8_ISSUE_B0(S)                                                                                               \
        T8_BAR() T8_LGKM0() T8_PRIO1() T8_MFMA(0, 2, 1) T8_MFMA(1, 2, 1) T8_PRIO0() T8_BAR()                         \
        T8_ISSUE_A0(S)                                                                                               \
        T8_VMCNT(4)                                                                                                          \
        T8_BAR() T8_PRIO1() T8_MFMA(1, 0, 2) T8_PRIO0() T8_BAR()                                                     \
    }

    // prologue: K-tile 0 complete into buffer 0, then the pieces of K-tile 1 the steady state would have issued by now
    if constexpr (BN == 256) {
        T8_ISSUE_A0(0) T8_ISSUE_B0(0) T8_ISSUE_A1(0) T8_ISSUE_B1(0)
        T8_ISSUE_B0(1) T8_ISSUE_A0(1) T8_ISSUE_A1(1)
        T8_VMCNT(6)
    } else {
        T8_ISSUE_A0(0) T8_ISSUE_B0(0) T8_ISSUE_A1(0) T8_ISSUE_B1(0)
        T8_ISSUE_B0(1) T8_ISSUE_A0(1)
        T8_VMCNT(4)
    }
    if (p.stagger_groups > 1) {
        // the prologue's DMA is in flight; this workgroup's group waits its share of the stagger before the first K-tile
        const int grp_ = (blockIdx.x >> 3) % p.stagger_groups;
        const unsigned long long t0_ = wall_clock64(), dt_ = (unsigned long long)grp_ * (unsigned)p.stagger_ticks;
        while (wall_clock64() - t0_ < dt_) __builtin_amdgcn_s_sleep(16);
    }
    T8_BAR()

    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        if (wr == 1) { T8_BAR() }             // the second half of the workgroup runs one barrier behind ...
        for (int kt = 0; kt < nk; kt += 2) {
            if constexpr (BN == 256) { T8_KTILE_256(0) T8_KTILE_256(1) }
            else { T8_KTILE_192(0) T8_KTILE_192(1) }
        }
        if (wr == 0) { T8_BAR() }             // ... and both halves run their epilogues side by side
        int tm, tn;
        tile_of_index(p, tile, ntiles, tm, tn);
        // which epilogue: the LDS-transposed one wins where row operands are LOADED (gated residual: FFN2 -4.5 %, out-projection
        // -2...4 %) and is level or better for the plain one; the GELU epilogue is bound by its two transcendentals per element and
        // pays the LDS round trip on top (+1...2 %), the qk-LayerNorm epilogue pays it and the 8-lane DPP reductions (+2.6 % on the
        // QKV pair in the model): those two keep the register-layout form (profiles/r4_gemm_epilogue_ablation.txt).  Each form
        // holds the code of its own epilogues only (static_assert in both).
        constexpr bool lds_epi = EPI != 1 && EPI != 4;
        if constexpr (lds_epi) t8_epilogue_lds<BN, EPI, MB>(p, acc, tm * BM + wr * (BM / 2), tn * BN + wc * (BN / 4), lane, smem + SCR + wave * 4096);
        else t8_epilogue<BN, EPI, MB>(p, acc, tm * BM + wr * (BM / 2), tn * BN + wc * (BN / 4), lane);
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < MB; ++b)
#pragma unroll
                for (int c = 0; c < NBW; ++c) acc[a][b][c] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
