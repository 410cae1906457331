// Development build only (-DVG_DEV, libvilgod_hip_dev.so): included by vit_dev_launchers.inc in place.  superseded K-step-32 ping-pong kernel: kept for the cycle-stamp tools (tools/dev), not in the product library
// ---------------------------------------------------------------------------------------------
// Ping-pong GEMM: 256 x 256 x 32 tiles, 8 waves = two groups of four (group = 128-row half of the tile, one wave of each
// group per SIMD), each wave 128 (m) x 64 (n).  A PHASE is one k16 sub-step of one wave: LOAD segment (6 ds_read_b128 for
// this sub-step's fragments + 2 LDS-DMA pieces of a tile several K-steps ahead), s_barrier, MFMA segment (8
// v_mfma_f32_32x32x16_f16 under s_setprio 1), s_barrier.  Group 1 runs ONE BARRIER behind group 0, so on every SIMD one
// wave's MFMA segment overlaps the other wave's LOAD segment: an LDS-DMA piece costs its issuing wave 60-185 cycles
// (MI355X_MICROARCH.md, cycle constants), which a lock-step schedule pays with an idle MFMA pipe.
// Ring of STAGES tiles (32 KB each: X rows 16 KB | W rows 16 KB).  Flat phase p = 2 kt + s issues half-tile q = p + LEAD
// (q even = X rows of tile q/2, odd = W rows), LEAD = 2 STAGES - 3: the slot's previous tile was last read two phases
// earlier by either group (WAR), and the counted wait for tile kt+1 (vmcnt = 2 (LEAD - 2) pieces may stay in flight) sits
// in the LOAD segment of phase (kt, 1), one full barrier before any wave reads that tile (RAW).
template <int EPI, int STAGES, bool TRACE = false, int PH = 2>
__global__ __launch_bounds__(512, 1) void k_gemm_f16_pp(const f16* __restrict__ X, const f16* __restrict__ Wt,
                                                        const float* __restrict__ bias, void* __restrict__ Cout,
                                                        float* __restrict__ resid, int M, int N, int K, int ldc, int cw,
                                                        long long* __restrict__ trace) {
    constexpr int BM = 256, BN = 256, NT = 512, TM = 4, TN = 2;
    constexpr int STAGE_BYTES = (BM + BN) * 64, W_OFF = BM * 64;
    constexpr int LEAD = 2 * STAGES - 3;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ntm = M / BM;
    const int t = xcd_remap(blockIdx.x, gridDim.x);
    const int per_chunk = ntm * cw;
    const int chunk = t / per_chunk, tc = t - chunk * per_chunk;
    const int tm = tc / cw, tn = chunk * cw + (tc - tm * cw);
    const int m0 = tm * BM, n0 = tn * BN;
    const int grp = wave >> 2, wn = wave & 3;

    // DMA: this wave stages rows [wave*32, +32) of the X half and of the W half (2 pieces of 16 rows each)
    const int l2 = lane >> 2, pslot = lane & 3;
    const int R0 = wave * 32 + l2, R1 = R0 + 16;
    const f16* xs0 = X + (size_t)(m0 + R0) * K + (pslot ^ ((R0 >> 2) & 3)) * 8;
    const f16* xs1 = X + (size_t)(m0 + R1) * K + (pslot ^ ((R1 >> 2) & 3)) * 8;
    const f16* ws0 = Wt + (size_t)(n0 + R0) * K + (pslot ^ ((R0 >> 2) & 3)) * 8;
    const f16* ws1 = Wt + (size_t)(n0 + R1) * K + (pslot ^ ((R1 >> 2) & 3)) * 8;
    char* const dma_base = smem + wave * 2048;
#define PP_ISSUE_X(TILE)                                                                                      \
    do {                                                                                                      \
        char* sb_ = dma_base + ((TILE) % STAGES) * STAGE_BYTES;                                               \
        __builtin_amdgcn_global_load_lds((glb_void*)(xs0 + (size_t)(TILE) * GK), (lds_void*)sb_, 16, 0, 0);  \
        __builtin_amdgcn_global_load_lds((glb_void*)(xs1 + (size_t)(TILE) * GK), (lds_void*)(sb_ + 1024), 16, 0, 0); \
    } while (0)
#define PP_ISSUE_W(TILE)                                                                                      \
    do {                                                                                                      \
        char* sb_ = dma_base + ((TILE) % STAGES) * STAGE_BYTES + W_OFF;                                       \
        __builtin_amdgcn_global_load_lds((glb_void*)(ws0 + (size_t)(TILE) * GK), (lds_void*)sb_, 16, 0, 0);  \
        __builtin_amdgcn_global_load_lds((glb_void*)(ws1 + (size_t)(TILE) * GK), (lds_void*)(sb_ + 1024), 16, 0, 0); \
    } while (0)

    f32x16 acc[TN][TM];
#pragma unroll
    for (int ni = 0; ni < TN; ++ni)
#pragma unroll
        for (int mi = 0; mi < TM; ++mi)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[ni][mi][r] = 0.f;

    const int r31 = lane & 31, hh = lane >> 5;
    const int sw = (r31 >> 2) & 3;
    const int xrow = (grp * 128 + r31) * 64, wrow = W_OFF + (wn * 64 + r31) * 64;
    const int po0 = ((0 + hh) ^ sw) * 16, po1 = ((2 + hh) ^ sw) * 16;
    const int nk = K / GK;            // host guarantees nk >= STAGES
    const int nh = 2 * nk;            // half-tiles

    f16x8 fa[TN], fb[TM];
#define PP_READ(SB, PO)                                                                      \
    _Pragma("unroll") for (int ni = 0; ni < TN; ++ni) fa[ni] = *(const f16x8*)((SB) + wrow + ni * 2048 + (PO)); \
    _Pragma("unroll") for (int mi = 0; mi < TM; ++mi) fb[mi] = *(const f16x8*)((SB) + xrow + mi * 2048 + (PO));
#define PP_MMA()                                                                             \
    __builtin_amdgcn_s_setprio(1);                                                           \
    _Pragma("unroll") for (int ni = 0; ni < TN; ++ni)                                        \
        _Pragma("unroll") for (int mi = 0; mi < TM; ++mi)                                    \
            acc[ni][mi] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[ni], fb[mi], acc[ni][mi], 0, 0, 0); \
    __builtin_amdgcn_s_setprio(0);
#define PP_BAR()                                  \
    __builtin_amdgcn_sched_barrier(0);            \
    __builtin_amdgcn_s_barrier();                 \
    __builtin_amdgcn_sched_barrier(0);
    // at most `newer` HALF-tiles issued after the wanted tile may stay in flight (2 pieces each)
#define PP_WAIT(newer)                                                                       \
    do {                                                                                     \
        const int nw_ = (newer);                                                             \
        if (nw_ >= LEAD - 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * (LEAD - 2)) : "memory"); \
        else if (nw_ == 6) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");                 \
        else if (nw_ == 5) asm volatile("s_waitcnt vmcnt(10)" ::: "memory");                 \
        else if (nw_ == 4) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");                  \
        else if (nw_ == 3) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");                  \
        else if (nw_ == 2) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");                  \
        else if (nw_ == 1) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");                  \
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                \
    } while (0)

    long long tr_wait = 0, tr_bar = 0, tr_t0 = 0, tr_load = 0, tr_mma = 0, tr_w0 = 0;
    if (TRACE) tr_w0 = wall_clock64();
  if (PH == 1) {
    // one phase per K-step: LOAD = 12 ds_reads + 4 DMA pieces (tile kt + D) + counted wait for tile kt+1; 16 MFMAs
    constexpr int D = STAGES - 2;
    f16x8 fa1[TN], fb1[TM];
#pragma unroll
    for (int q = 0; q < D; ++q) { PP_ISSUE_X(q); PP_ISSUE_W(q); }
    PP_WAIT(2 * (D - 1));
    PP_BAR()
    if (grp == 1) { PP_BAR() }
    if (TRACE) tr_t0 = clock64();
    for (int kt = 0; kt < nk; ++kt) {
        const char* sb = smem + (kt % STAGES) * STAGE_BYTES;
        long long c0 = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0;
        if (TRACE) c0 = clock64();
        PP_READ(sb, po0)
#pragma unroll
        for (int ni = 0; ni < TN; ++ni) fa1[ni] = *(const f16x8*)(sb + wrow + ni * 2048 + po1);
#pragma unroll
        for (int mi = 0; mi < TM; ++mi) fb1[mi] = *(const f16x8*)(sb + xrow + mi * 2048 + po1);
        if (kt + D < nk) { PP_ISSUE_X(kt + D); PP_ISSUE_W(kt + D); }
        if (TRACE) c1 = clock64();
        if (kt + 1 < nk) {
            const int newest = (kt + D < nk - 1) ? kt + D : nk - 1;
            PP_WAIT(2 * (newest - (kt + 1)));
        }
        if (TRACE) c2 = clock64();
        PP_BAR()
        if (TRACE) c3 = clock64();
        PP_MMA()
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int ni = 0; ni < TN; ++ni)
#pragma unroll
            for (int mi = 0; mi < TM; ++mi)
                acc[ni][mi] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa1[ni], fb1[mi], acc[ni][mi], 0, 0, 0);
        __builtin_amdgcn_s_setprio(0);
        if (TRACE) c4 = clock64();
        PP_BAR()
        if (TRACE) { const long long c5 = clock64(); tr_load += c1 - c0; tr_wait += c2 - c1; tr_bar += (c3 - c2) + (c5 - c4); tr_mma += c4 - c3; }
    }
  } else {
    // prologue: half-tiles 0 .. LEAD-1, then tile 0 (halves 0,1) must have landed
#pragma unroll
    for (int q = 0; q < LEAD; ++q) {
        if (q & 1) PP_ISSUE_W(q >> 1); else PP_ISSUE_X(q >> 1);
    }
    PP_WAIT(LEAD - 2);
    PP_BAR()
    if (grp == 1) { PP_BAR() }          // group 1 runs one barrier behind group 0
    if (TRACE) tr_t0 = clock64();
    for (int kt = 0; kt < nk; ++kt) {
        const char* sb = smem + (kt % STAGES) * STAGE_BYTES;
        long long c0 = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0;
        // ---- phase (kt, 0): LEAD is odd -> half-tile 2kt+LEAD is the W half of tile kt + (LEAD-1)/2
        if (TRACE) c0 = clock64();
        PP_READ(sb, po0)
        if (2 * kt + LEAD < nh) PP_ISSUE_W(kt + (LEAD >> 1));
        if (TRACE) c1 = clock64();
        PP_BAR()
        if (TRACE) c2 = clock64();
        PP_MMA()
        if (TRACE) c3 = clock64();
        PP_BAR()
        if (TRACE) { c4 = clock64(); tr_load += c1 - c0; tr_bar += (c2 - c1) + (c4 - c3); tr_mma += c3 - c2; }
        // ---- phase (kt, 1): half-tile 2kt+1+LEAD is the X half of tile kt + (LEAD+1)/2
        if (TRACE) c0 = clock64();
        PP_READ(sb, po1)
        if (2 * kt + 1 + LEAD < nh) PP_ISSUE_X(kt + ((LEAD + 1) >> 1));
        if (TRACE) c1 = clock64();
        if (kt + 1 < nk) {
            // newest half-tile issued so far: min(2kt+1+LEAD, nh-1); tile kt+1 = halves 2kt+2, 2kt+3
            const int newest = (2 * kt + 1 + LEAD < nh - 1) ? 2 * kt + 1 + LEAD : nh - 1;
            PP_WAIT(newest - (2 * kt + 3));
        }
        if (TRACE) { c2 = clock64(); tr_load += c1 - c0; tr_wait += c2 - c1; }
        PP_BAR()
        if (TRACE) c3 = clock64();
        PP_MMA()
        if (TRACE) c4 = clock64();
        PP_BAR()
        if (TRACE) { const long long c5 = clock64(); tr_bar += (c3 - c2) + (c5 - c4); tr_mma += c4 - c3; }
    }
  }
    if (grp == 0) { PP_BAR() }
#undef PP_ISSUE_X
#undef PP_ISSUE_W
#undef PP_READ
#undef PP_MMA
#undef PP_BAR
#undef PP_WAIT
    long long tr_t1 = 0;
    if (TRACE) tr_t1 = clock64();
    // ---- epilogue through LDS (the whole ring is free: every DMA landed, every fragment is in registers) ----
    // The tile is laid down with its 16-byte chunks XOR-swizzled by (row & 31) instead of row padding, so a full
    // 256 x 256 fp16 tile (128 KB) or a 128-row fp32 half fits the ring exactly and both the lane-per-row writes and
    // the row-contiguous reads are bank-conflict free.  Bias / QuickGELU are applied in registers (a lane's n is fixed).
    __syncthreads();
    if (EPI == EPI_BIAS || EPI == EPI_BIAS_GELU) {
#pragma unroll
        for (int ni = 0; ni < TN; ++ni)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int nloc = wn * 64 + ni * 32 + 8 * g + 4 * hh;
                const float4 b4 = *(const float4*)(bias + n0 + nloc);
                const int ch = nloc >> 3;
#pragma unroll
                for (int mi = 0; mi < TM; ++mi) {
                    const int m = grp * 128 + mi * 32 + r31;
                    float v[4] = {acc[ni][mi][4 * g] + b4.x, acc[ni][mi][4 * g + 1] + b4.y, acc[ni][mi][4 * g + 2] + b4.z,
                                  acc[ni][mi][4 * g + 3] + b4.w};
                    f16x4 h4;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float x = v[e];
                        if (EPI == EPI_BIAS_GELU) x = x * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(x * QGELU_C));   // QuickGELU (model.py:166-168)
                        h4[e] = (f16)x;
                    }
                    *(f16x4*)(smem + m * 512 + ((ch ^ r31) << 4) + hh * 8) = h4;
                }
            }
        __syncthreads();
        const int j = tid & 31, rr = tid >> 5;
#pragma unroll 4
        for (int pass = 0; pass < 16; ++pass) {
            const int m = pass * 16 + rr;
            const f16x8 v = *(const f16x8*)(smem + m * 512 + j * 16);
            *(f16x8*)((f16*)Cout + (size_t)(m0 + m) * ldc + n0 + ((j ^ (m & 31)) << 3)) = v;
        }
    } else {
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            if (half) __syncthreads();
            if (grp == half) {
#pragma unroll
                for (int ni = 0; ni < TN; ++ni)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int nloc = wn * 64 + ni * 32 + 8 * g + 4 * hh;
                        float4 b4 = make_float4(0.f, 0.f, 0.f, 0.f);
                        if (EPI == EPI_BIAS_RESID) b4 = *(const float4*)(bias + n0 + nloc);
                        const int ch = nloc >> 2;
#pragma unroll
                        for (int mi = 0; mi < TM; ++mi) {
                            const int m = mi * 32 + r31;
                            *(float4*)(smem + m * 1024 + ((ch ^ r31) << 4)) =
                                make_float4(acc[ni][mi][4 * g] + b4.x, acc[ni][mi][4 * g + 1] + b4.y,
                                            acc[ni][mi][4 * g + 2] + b4.z, acc[ni][mi][4 * g + 3] + b4.w);
                        }
                    }
            }
            __syncthreads();
            const int j = tid & 63, rr = tid >> 6;
#pragma unroll
            for (int p8 = 0; p8 < 2; ++p8) {
                // eight residual loads in flight before the first store (a load / add / store loop serialises on aliasing)
                float4 x4[8];
                if (EPI == EPI_BIAS_RESID) {
#pragma unroll
                    for (int q = 0; q < 8; ++q) {
                        const int m = (p8 * 8 + q) * 8 + rr;
                        x4[q] = *(const float4*)(resid + (size_t)(m0 + half * 128 + m) * ldc + n0 + ((j ^ (m & 31)) << 2));
                    }
                }
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const int m = (p8 * 8 + q) * 8 + rr;
                    float4 v = *(const float4*)(smem + m * 1024 + j * 16);
                    const size_t off = (size_t)(m0 + half * 128 + m) * ldc + n0 + ((j ^ (m & 31)) << 2);
                    if (EPI == EPI_BIAS_RESID) {
                        v.x += x4[q].x; v.y += x4[q].y; v.z += x4[q].z; v.w += x4[q].w;
                        *(float4*)(resid + off) = v;
                    } else {
                        *(float4*)((float*)Cout + off) = v;
                    }
                }
            }
        }
    }
    if (TRACE) {
        const long long tr_t2 = clock64();
        if (lane == 0 && trace) {
            long long* o = trace + ((size_t)blockIdx.x * 8 + wave) * 8;
            o[0] = tr_t1 - tr_t0; o[1] = tr_wait; o[2] = tr_bar; o[3] = tr_t2 - tr_t1; o[4] = tr_load; o[5] = tr_mma; o[6] = wave; o[7] = wall_clock64() - tr_w0;
        }
    }
}

