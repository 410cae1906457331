// Part of vit.hip (included in place): the projection-GEMM kernels.  k_gemm_f16, k_gemm_f32, k_gemm_f32_mfma; k_gemm_f16_pp64;
// k_gemm_f16_w4 (its K loop: gemm_w4_loop.inc) and k_splitk_resid.  Launchers and the choice between them: vit_gemm_launch.inc.

// QuickGELU x * sigmoid(1.702 x) (model.py:166-168) as x / (1 + 2^(x * QGELU_C)): one multiply in front of v_exp_f32 instead of two
#define QGELU_C (-1.702f * 1.4426950408889634f)
enum { EPI_BIAS = 0, EPI_BIAS_GELU = 1, EPI_BIAS_RESID = 2, EPI_NONE_F32 = 3,
       EPI_BIAS_RESID_H = 4,     // 4: fp16 residual stream (k_gemm_f16_pp64 only): resid_h = f16(resid_h + f16(acc + bias))
       EPI_BIAS_RESID_HL = 5 };  // 5: the residual stream as an fp16 PAIR (k_gemm_f16_w4 only, LN = 2): x = hi + lo, hi = the fp16 copy the next
                                 //    GEMM reads (ln_x16), lo = f16(x - hi) (`resid`, as f16*): 22 bits of x in 4 bytes, read 4 + written 4 per element
                                 //    instead of read 4 + written 6

// ---------------------------------------------------------------------------------------------
// XCD-aware tile order: consecutive hardware block ids are dealt round-robin to the 8 XCDs; give each
// XCD a contiguous run of tiles so the column tiles that share one activation row-tile hit one L2.
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
    int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, s = bid >> 3;
    int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + s;
}

// ---------------------------------------------------------------------------------------------
// fp16 MFMA GEMM:  C[m][n] = sum_k X[m][k] * Wt[n][k]  (+ epilogue).  M%256==0, N%128==0, K%32==0.
// The MFMA computes the TRANSPOSED tile (A operand = weight rows, B operand = activation rows) so a
// lane owns one output row m and 4-wide runs of consecutive n: vector loads/stores in the epilogue.
#define GBM 256                             // block tile: 256 (tokens) x 128 (features), K-step 32
#define GBN 128
#define GK 32
#define G_STAGES 3
#define G_STAGE_BYTES 24576                 // one stage: X tile 16 KB + W tile 8 KB, rows of 64 B, linear
#define G_W_OFF 16384
#define G_EPI_LD 132                        // epilogue tile row stride in floats (128 + 4: conflict-free b128 writes)
#define G_LDS_BYTES (G_STAGES * G_STAGE_BYTES)   // 73,728 B (>= 128*132*4 = 67,584 B half-tile) -> 2 workgroups / CU

typedef __attribute__((address_space(3))) void lds_void;
typedef const __attribute__((address_space(1))) void glb_void;

// fp16 MFMA GEMM:  C[m][n] = sum_k X[m][k] * Wt[n][k]  (+ epilogue).  M%256==0, N%128==0, K%32==0.
//  * 8 waves (4 x 2), each a 64x64 sub-tile = 2x2 v_mfma_f32_32x32x16_f16; the MFMA computes the TRANSPOSED tile
//    (A operand = weight rows, B operand = activation rows) so a lane owns one output row.
//  * staging by LDS-DMA (global_load_lds, 16 B per lane): no staging registers, no ds_write pass.  The DMA writes
//    LDS linearly (wave-uniform base + lane*16), so the bank-conflict swizzle is applied to the per-lane SOURCE
//    address and again to the ds_read address (guide rule 21): 16-B chunk c of the 64-B row r sits at slot
//    c ^ ((r>>2)&3).
//  * 3 stages, TWO tiles in flight: per K-step one counted s_waitcnt vmcnt(3) (this wave's 3 newest DMAs = the next
//    tile may stay in flight) + one raw s_barrier; the DMA for tile k+2 is issued right after the barrier.
//  * 72 KB of LDS and <= 128 VGPRs -> TWO workgroups per CU: one block's barrier waits and epilogue overlap the other's
//    MFMAs (ablation: compute-only and DMA-only each take ~60 % of the fused time when run alone in one block).
//  * epilogue through LDS in two 128-row halves: accumulators -> [128][128] f32 tile -> whole rows, 16 B per lane,
//    fused bias / QuickGELU / residual update.  ldc = row stride of C (qkv uses a padded stride: 4608-B rows alias
//    in the memory channels and cost +20 %).
template <int EPI, int VAR = 0>
__global__ __launch_bounds__(512, 2) void k_gemm_f16(const f16* __restrict__ X, const f16* __restrict__ Wt,
                                                     const float* __restrict__ bias, void* __restrict__ Cout,
                                                     float* __restrict__ resid, int M, int N, int K, int ldc, int cw) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // tile order: column CHUNKS of cw tiles (<= ~2.4 MB of weights, so the chunk stays in one XCD's 4 MB L2 next to the
    // streaming activations), inside a chunk row-tile major; each XCD walks a contiguous run of this order.
    const int ntm = M / GBM;
    const int t = xcd_remap(blockIdx.x, gridDim.x);
    const int per_chunk = ntm * cw;
    const int chunk = t / per_chunk, tc = t - chunk * per_chunk;
    const int tm = tc / cw, tn = chunk * cw + (tc - tm * cw);
    const int m0 = tm * GBM, n0 = tn * GBN;
    const int wm = wave >> 1, wn = wave & 1;          // 4 x 2 waves, 64x64 each

    // ---- DMA addressing: a 1-KB instruction covers 16 rows x 64 B.  This wave fills X rows [wave*32, +32) (2
    //      instructions) and W rows [wave*16, +16) (1) ----
    const int l2 = lane >> 2, pslot = lane & 3;
    const f16* xsrc[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int R = wave * 32 + q * 16 + l2;
        xsrc[q] = X + (size_t)(m0 + R) * K + (pslot ^ ((R >> 2) & 3)) * 8;
    }
    const int RW = wave * 16 + l2;
    const f16* wsrc = Wt + (size_t)(n0 + RW) * K + (pslot ^ ((RW >> 2) & 3)) * 8;
    auto issue = [&](int kt, int stage) {
        char* sb = smem + stage * G_STAGE_BYTES;
        __builtin_amdgcn_global_load_lds((glb_void*)(xsrc[0] + (size_t)kt * GK), (lds_void*)(sb + (wave * 32) * 64), 16, 0, 0);
        __builtin_amdgcn_global_load_lds((glb_void*)(xsrc[1] + (size_t)kt * GK), (lds_void*)(sb + (wave * 32 + 16) * 64), 16, 0, 0);
        __builtin_amdgcn_global_load_lds((glb_void*)(wsrc + (size_t)kt * GK), (lds_void*)(sb + G_W_OFF + (wave * 16) * 64), 16, 0, 0);
    };

    f32x16 acc00, acc01, acc10, acc11;   // acc[ni][mi]
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc00[r] = 0.f; acc01[r] = 0.f; acc10[r] = 0.f; acc11[r] = 0.f; }

    const int r31 = lane & 31, hh = lane >> 5;
    const int sw = (r31 >> 2) & 3;
    const int xrow = (wm * 64 + r31) * 64, wrow = G_W_OFF + (wn * 64 + r31) * 64;
    const int nk = K / GK;
    issue(0, 0);
    if (nk > 1) issue(1, 1);
    for (int kt = 0; kt < nk; ++kt) {
        // tile kt must have landed; the 3 newest DMAs of this wave (tile kt+1) may stay in flight
        if (kt + 1 < nk) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();    // every wave's part of tile kt is in LDS; stage (kt+2)%3 is no longer read
        if (VAR != 1 && kt + 2 < nk) issue(kt + 2, (kt + 2) % G_STAGES);
        const char* sb = smem + (kt % G_STAGES) * G_STAGE_BYTES;
        if (VAR == 2) continue;
#pragma unroll
        for (int s = 0; s < GK / 16; ++s) {
            const int po = ((2 * s + hh) ^ sw) * 16;
            f16x8 fa0 = *(const f16x8*)(sb + wrow + po);
            f16x8 fa1 = *(const f16x8*)(sb + wrow + 32 * 64 + po);
            f16x8 fb0 = *(const f16x8*)(sb + xrow + po);
            f16x8 fb1 = *(const f16x8*)(sb + xrow + 32 * 64 + po);
            acc00 = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa0, fb0, acc00, 0, 0, 0);
            acc01 = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa0, fb1, acc01, 0, 0, 0);
            acc10 = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa1, fb0, acc10, 0, 0, 0);
            acc11 = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa1, fb1, acc11, 0, 0, 0);
        }
    }
    if (VAR == 3) { if (acc00[0] + acc01[1] + acc10[2] + acc11[3] == 12345.f) ((float*)Cout)[0] = 1.f; return; }
    // ---- epilogue through LDS, two halves of 128 rows (waves wm = 0,1 hold rows 0..127; wm = 2,3 rows 128..255) ----
    float* ct = (float*)smem;
    f32x16 acc[2][2] = {{acc00, acc01}, {acc10, acc11}};
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        __syncthreads();
        if ((wm >> 1) == half) {
#pragma unroll
            for (int mi = 0; mi < 2; ++mi) {
                const int m = (wm & 1) * 64 + mi * 32 + r31;     // lane owns row m; register r -> n = (r&3) + 8*(r>>2) + 4*hh
#pragma unroll
                for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int n = wn * 64 + ni * 32 + 8 * g + 4 * hh;
                        *(float4*)(ct + m * G_EPI_LD + n) = make_float4(acc[ni][mi][4 * g], acc[ni][mi][4 * g + 1],
                                                                        acc[ni][mi][4 * g + 2], acc[ni][mi][4 * g + 3]);
                    }
            }
        }
        __syncthreads();
        const int mh = m0 + half * 128;
        if (EPI == EPI_BIAS || EPI == EPI_BIAS_GELU) {
            // f16 output: a row of 128 values = 256 B = 16 lanes x 16 B; 32 rows per pass
            const int cn = (tid & 15) * 8, rr = tid >> 4;
            const float4 b0 = *(const float4*)(bias + n0 + cn), b1 = *(const float4*)(bias + n0 + cn + 4);
            const float bb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
            for (int pass = 0; pass < 4; ++pass) {
                const int m = pass * 32 + rr;
                const float4 v0 = *(const float4*)(ct + m * G_EPI_LD + cn), v1 = *(const float4*)(ct + m * G_EPI_LD + cn + 4);
                float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
                f16x8 h8;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    float x = v[e] + bb[e];
                    if (EPI == EPI_BIAS_GELU) x = x * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(x * QGELU_C));   // QuickGELU (model.py:166-168)
                    h8[e] = (f16)x;
                }
                *(f16x8*)((f16*)Cout + (size_t)(mh + m) * ldc + n0 + cn) = h8;
            }
        } else {
            // f32 output / residual update: a row of 128 floats = 512 B = 32 lanes x 16 B; 16 rows per pass
            const int cn = (tid & 31) * 4, rr = tid >> 5;
            float4 b4 = make_float4(0.f, 0.f, 0.f, 0.f);
            if (EPI == EPI_BIAS_RESID) b4 = *(const float4*)(bias + n0 + cn);
#pragma unroll
            for (int pass = 0; pass < 8; ++pass) {
                const int m = pass * 16 + rr;
                float4 v = *(const float4*)(ct + m * G_EPI_LD + cn);
                if (EPI == EPI_BIAS_RESID) {
                    float* p = resid + (size_t)(mh + m) * ldc + n0 + cn;
                    const float4 x4 = *(const float4*)p;
                    v.x += b4.x + x4.x; v.y += b4.y + x4.y; v.z += b4.z + x4.z; v.w += b4.w + x4.w;
                    *(float4*)p = v;
                } else {
                    *(float4*)((float*)Cout + (size_t)(mh + m) * ldc + n0 + cn) = v;
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// fp32 parity-mode GEMM (VALU): 64x64 tile, 256 threads, 4x4 micro-tile, same epilogues.
template <int EPI>
__global__ __launch_bounds__(256) void k_gemm_f32(const float* __restrict__ X, const float* __restrict__ Wt,
                                                  const float* __restrict__ bias, float* __restrict__ Cout,
                                                  float* __restrict__ resid, int M, int N, int K) {
    __shared__ float Xs[16][64 + 4];
    __shared__ float Ws[16][64 + 4];
    const int tid = threadIdx.x;
    const int ntn = N / 64;
    const int tm = blockIdx.x / ntn, tn = blockIdx.x - tm * ntn;
    const int m0 = tm * 64, n0 = tn * 64;
    const int ty = tid >> 4, tx = tid & 15;
    float acc[4][4] = {};
    for (int k0 = 0; k0 < K; k0 += 16) {
        // 64 rows x 16 k per operand = 1024 values, 4 per thread
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            int c = tid + 256 * i, row = c >> 4, kk = c & 15;
            Xs[kk][row] = X[(size_t)(m0 + row) * K + k0 + kk];
            Ws[kk][row] = Wt[(size_t)(n0 + row) * K + k0 + kk];
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
            float a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                a[i] = Xs[kk][ty * 4 + i];
                b[i] = Ws[kk][tx * 4 + i];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(a[i], b[j], acc[i][j]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + ty * 4 + i;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = n0 + tx * 4 + j;
            float v = acc[i][j];
            if (EPI != EPI_NONE_F32) v += bias[n];
            if (EPI == EPI_BIAS_GELU) v = v / (1.0f + expf(-1.702f * v));
            if (EPI == EPI_BIAS_RESID)
                resid[(size_t)m * N + n] += v;
            else
                Cout[(size_t)m * N + n] = v;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// fp32 parity-mode GEMM on the matrix cores (round 4): v_mfma_f32_32x32x2_f32 -- f32 in, f32 accumulate, each instruction two exact
// fused multiply-adds per output element in k order, i.e. the same fmaf chain over ascending k as k_gemm_f32 above (the tower's
// numbers do not change), at the vector-ALU peak rate but with 1/32 of the LDS reads per FLOP of the 4 x 4 micro-tile kernel.
// 128 x 128 tile, 256 threads = 2 x 2 waves of 64 x 64 (2 x 2 blocks of 32 x 32: 64 accumulator registers), K-step 16.
// LDS tiles are k-major ([16][128 + 4] floats per operand): lane l reads A[k0 + l / 32][row l % 32] -- 32 consecutive floats per
// half-wave, conflict-free.  The next K-step's global loads (a float4 along k per thread and operand half) are in registers while the
// current one is multiplied.  D layout of the 32 x 32 instruction: register j of lane l = token 8 (j / 4) + 4 (l / 32) + j % 4,
// feature l % 32 -> a store instruction writes two 128-byte row segments.
typedef float f32x16m __attribute__((ext_vector_type(16)));
#define GF_LD 132
template <int EPI>
__global__ __launch_bounds__(256) void k_gemm_f32_mfma(const float* __restrict__ X, const float* __restrict__ Wt,
                                                       const float* __restrict__ bias, float* __restrict__ Cout,
                                                       float* __restrict__ resid, int M, int N, int K) {
    __shared__ float As[16 * GF_LD];
    __shared__ float Bs[16 * GF_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ntn = N / 128;
    const int tm = blockIdx.x / ntn, tn = blockIdx.x - tm * ntn;
    const int m0 = tm * 128, n0 = tn * 128;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
    const int l32 = lane & 31, lk = lane >> 5;
    // staging: thread t moves rows (t >> 2) and (t >> 2) + 64 of each operand, k quad t & 3
    const int srow = tid >> 2, skq = (tid & 3) * 4;
    float4 xa, xb, wa, wb;
    auto fetch = [&](int k0) {
        xa = *(const float4*)(X + (size_t)(m0 + srow) * K + k0 + skq);
        xb = *(const float4*)(X + (size_t)(m0 + srow + 64) * K + k0 + skq);
        wa = *(const float4*)(Wt + (size_t)(n0 + srow) * K + k0 + skq);
        wb = *(const float4*)(Wt + (size_t)(n0 + srow + 64) * K + k0 + skq);
    };
    auto stage = [&]() {
        const float xs[2][4] = {{xa.x, xa.y, xa.z, xa.w}, {xb.x, xb.y, xb.z, xb.w}};
        const float ws[2][4] = {{wa.x, wa.y, wa.z, wa.w}, {wb.x, wb.y, wb.z, wb.w}};
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                As[(skq + e) * GF_LD + srow + 64 * h] = xs[h][e];
                Bs[(skq + e) * GF_LD + srow + 64 * h] = ws[h][e];
            }
    };
    f32x16m acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    fetch(0);
    for (int k0 = 0; k0 < K; k0 += 16) {
        stage();
        __syncthreads();
        if (k0 + 16 < K) fetch(k0 + 16);
#pragma unroll
        for (int kk = 0; kk < 16; kk += 2) {
            float a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                a[i] = As[(kk + lk) * GF_LD + wm + 32 * i + l32];
                b[i] = Bs[(kk + lk) * GF_LD + wn + 32 * i + l32];
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int n = n0 + wn + 32 * j + l32;
            const float bn = EPI != EPI_NONE_F32 ? bias[n] : 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm + 32 * i + 8 * (r >> 2) + 4 * lk + (r & 3);
                float v = acc[i][j][r];
                if (EPI != EPI_NONE_F32) v += bn;
                if (EPI == EPI_BIAS_GELU) v = v / (1.0f + expf(-1.702f * v));
                if (EPI == EPI_BIAS_RESID)
                    resid[(size_t)m * N + n] += v;
                else
                    Cout[(size_t)m * N + n] = v;
            }
        }
}

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------------------
// K-step 64 (128-byte rows).  Measured with tools/micro/dma_rate.hip: LDS-DMA from L2-resident data streams at
// 39 B/clk/CU when a piece covers 16 rows x 64 B and at 64 B/clk/CU (the L1 peak) when it covers 8 rows x 128 B -- a
// 256 x 256 x 32 K-step needs 32 B/clk/CU at full MFMA rate, so 64-byte row segments leave the LOAD segment the
// longer one of the ping-pong pair.  Here a phase is one 64-wide K-tile (two k32 sub-steps, 64 MFMAs per wave):
//   LDS (all 160 KB): X ring 2 x 32 KB + W ring 3 x 32 KB; a row is 128 B, 16-byte chunk c of row r sits at c ^ ((r>>1)&7).
//   Group g reads X rows [128 g, +128) only -> it refills them itself (K-tile j+1 in LOAD_j, its slot was last read
//   in the group's own MMA_{j-1}).  W rows are read by both groups; group 1, which runs one barrier behind, is the
//   last reader of a W slot: W of K-tile j+2 goes into the slot of K-tile j-1, half by group 1 in its LOAD_j and half
//   by group 0 in its LOAD_{j+1} (3-deep ring -> at least one interval of lead).
//   The second k32 sub-step's fragments are read during the first sub-step's MFMAs into the registers those have
//   just consumed.  Every wave waits for its own pieces (vmcnt(0)) before the barrier that ends its MMA segment.
//
// LayerNorm folded into the GEMMs around it (LN = 1 / 2; ViT blocks, fp32 residual stream).  ln(x) W^T + b with
// ln(x) = (x - mean) * rstd * g + beta is  rstd * (x (g.W)^T - mean * c1) + c2,  c1[n] = sum_k g[k] W[n,k],
// c2[n] = b[n] + sum_k beta[k] W[n,k]:  the CONSUMER (LN = 1: in_proj, c_fc) multiplies the raw residual (as fp16) by the
// pre-scaled weights and applies the row statistics in its epilogue; the PRODUCER (LN = 2: out_proj, c_proj, whose epilogue
// holds the new residual row segments anyway) writes that fp16 copy and, per row and 256-column tile, (mean, sum of squared
// deviations from it) -- the consumer merges the K / 256 partials of a row (Chan et al.), so the variance is the two-pass
// variance, not E[x^2] - mean^2.  Saves the separate LayerNorm pass over the residual stream (295 MB per launch, 23 per frame).
struct LnPartial { float mean, m2; };
__device__ __forceinline__ float row256_sum(float v) {          // sum over the 64 lanes, fixed order: DPP inside rows of 16, then the four rows
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));    // quad_perm [1,0,3,2]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));    // quad_perm [2,3,0,1]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true));   // row_half_mirror
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, true));   // row_mirror
    const int b = __builtin_bit_cast(int, v);
    return (__builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 0)) + __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 16))) +
           (__builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 32)) + __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 48)));
}

// Measured and dropped (round 4): "RI" -- every lane loads the residual elements of its accumulator registers in the prologue, in
// front of the first LDS-DMA pieces, the MFMAs accumulate on top and the epilogue is write-only.  Launches interleaved on one box at
// M = 66560: out_proj 188 vs 177 us and c_proj 382 vs 366 us with the residual stream out of the memory-side cache (as in the
// pipeline), 157 vs 156 / 362 vs 360 with it cached; whole pipeline 65.1 vs 65.0 frames/s.  The residual epilogue is bound by the bytes
// all CUs move at the same time (510 MB per launch), not by the latency of its load -> add -> store rounds.
//
// SPLITK (round 4; EPI_NONE_F32 only): the workgroup computes K-tiles [part np / P, (part + 1) np / P) of tile blockIdx.x / P (row-major
// over the M / 256 x N / 256 tiles of THIS launch) and stores the raw fp32 accumulators as a dense 256 x 256 image at
// Cout + blockIdx.x * 65536 -- the partial sums of a split-K tail (launch_gemm_resid_tail below; k_splitk_resid adds them up).
template <int EPI, bool TRACE = false, bool PERSIST = false, int LN = 0, bool SPLITK = false>
__global__ __launch_bounds__(512, 1) void k_gemm_f16_pp64(const f16* __restrict__ X, const f16* __restrict__ Wt,
                                                          const float* __restrict__ bias, void* __restrict__ Cout,
                                                          float* __restrict__ resid, int M, int N, int K, int ldc, int cw,
                                                          long long* __restrict__ trace = nullptr,
                                                          const float* __restrict__ ln_c1 = nullptr, LnPartial* __restrict__ ln_stats = nullptr,
                                                          f16* __restrict__ ln_x16 = nullptr, int sk_parts = 1) {
    static_assert(!SPLITK || (EPI == EPI_NONE_F32 && !PERSIST && LN == 0), "split-K partials are raw fp32 tiles");
    constexpr int BM = 256, BN = 256, NT = 512, TM = 8, TN = 4;
    constexpr int XBUF = 32768, WBASE = 2 * XBUF, WBUF = 32768;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // wave id in an SGPR
    const int ntm = M / BM;
    const int grp = wave >> 2, wn = wave & 3;
    long long tr_entry = 0, tr_load = 0, tr_bar = 0, tr_mma = 0, tr_wait = 0, tr_t0 = 0, tr_w0 = 0, tr_main = 0, tr_w_entry = 0;
    if (TRACE) { tr_entry = clock64(); tr_w_entry = wall_clock64(); }
    // PERSIST: one workgroup per CU walks its XCD's contiguous run of tiles (slot s of G/8 takes tiles s, s + G/8, ...), which
    // removes the 1-2 us a CU idles between two workgroups; nothing of consecutive tiles overlaps (the registers are full).
    const int nt_all = ntm * (N / BN);
    const int xq = nt_all >> 3, xr_ = nt_all & 7, xcd = blockIdx.x & 7;
    const int xbase = (xcd < xr_) ? xcd * (xq + 1) : xr_ * (xq + 1) + (xcd - xr_) * xq;
    const int xcnt = xq + (xcd < xr_ ? 1 : 0);
    for (int ti = PERSIST ? (int)(blockIdx.x >> 3) : 0; ti < (PERSIST ? xcnt : 1); ti += PERSIST ? (int)(gridDim.x >> 3) : 1) {
    int lane = tid & 63;
    if (PERSIST) asm volatile("" : "+v"(lane));      // per-lane offsets are re-derived per tile instead of living through the epilogue
    const int t = PERSIST ? xbase + ti : xcd_remap(blockIdx.x, gridDim.x);
    const int per_chunk = ntm * cw;
    const int chunk = t / per_chunk, tc = t - chunk * per_chunk;
    int tm = tc / cw, tn = chunk * cw + (tc - tm * cw);
    int kt0 = 0, np = K / 64;                      // host guarantees K % 64 == 0 and np >= 2 (per part when SPLITK)
    if (SPLITK) {
        const int st_ = (int)blockIdx.x / sk_parts, part = (int)blockIdx.x - st_ * sk_parts, ntn_ = N / BN;
        tm = st_ / ntn_; tn = st_ - tm * ntn_;
        kt0 = part * np / sk_parts;
        np = (part + 1) * np / sk_parts - kt0;
    }
    const int m0 = tm * BM, n0 = tn * BN;

    // DMA pieces: 8 rows x 128 B; lane -> row l >> 3, chunk slot l & 7 (source chunk = slot ^ ((row >> 1) & 7))
    const int prow = lane >> 3, pslot = lane & 7;
    const int xr = grp * 128 + wn * 32 + prow;                         // + 8 i, i = 0..3
    auto issue_x = [&](int kt) {                                       // this group's X half of K-tile kt
        char* d = smem + (kt & 1) * XBUF + (grp * 128 + wn * 32) * 128;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = xr + 8 * i;
            const f16* sp = X + (size_t)(m0 + r) * K + (size_t)(kt0 + kt) * 64 + (pslot ^ ((r >> 1) & 7)) * 8;
            __builtin_amdgcn_global_load_lds((glb_void*)sp, (lds_void*)(d + i * 1024), 16, 0, 0);
        }
    };
    // W rows [128 h, +128) of K-tile kt, four pieces per wave.  Half 0 is issued by group 1 in LOAD_{kt-2}, half 1 by
    // group 0 in LOAD_{kt-1} (both after the slot's last reader, group 1's MMA_{kt-3}, has passed its barrier), which
    // balances the DMA work: 8 pieces per wave and phase in either group.
    auto issue_w = [&](int kt, int h) {
        char* d = smem + WBASE + (kt % 3) * WBUF + (h * 128 + wn * 32) * 128;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = h * 128 + wn * 32 + prow + 8 * i;
            const f16* sp = Wt + (size_t)(n0 + r) * K + (size_t)(kt0 + kt) * 64 + (pslot ^ ((r >> 1) & 7)) * 8;
            __builtin_amdgcn_global_load_lds((glb_void*)sp, (lds_void*)(d + i * 1024), 16, 0, 0);
        }
    };
    f32x4 acc[TN][TM];
#pragma unroll
    for (int ni = 0; ni < TN; ++ni)
#pragma unroll
        for (int mi = 0; mi < TM; ++mi) acc[ni][mi] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int r15 = lane & 15, q4 = lane >> 4;
    const int swz = (r15 >> 1) & 7;
    const int xo0 = (grp * 128 + r15) * 128 + ((q4 ^ swz) << 4), xo1 = (grp * 128 + r15) * 128 + (((4 + q4) ^ swz) << 4);
    const int wo0 = (wn * 64 + r15) * 128 + ((q4 ^ swz) << 4), wo1 = (wn * 64 + r15) * 128 + (((4 + q4) ^ swz) << 4);
    const unsigned lds0 = (unsigned)(unsigned long)(__attribute__((address_space(3))) char*)smem;     // LDS byte address of the rings (inline-asm reads)
    // folded LayerNorm, consumer side: thread t < 256 merges the K / 256 partials of tile row t into (mean, rstd) here, where the
    // loads' latency hides behind the prologue's DMA (in the epilogue it cost ~7 us per tile), and carries two registers
    float2 ln_row = make_float2(0.f, 0.f);
    LnPartial pt[4] = {};
    const int nst = K >> 8;                        // <= 4 (width <= 1024)
    if (LN == 1 && tid < BM) {
        const LnPartial* sp = ln_stats + (size_t)(m0 + tid) * nst;
#pragma unroll
        for (int t = 0; t < 4; ++t) pt[t] = t < nst ? sp[t] : LnPartial{0.f, 0.f};
    }

#define PP_BAR()                                  \
    __builtin_amdgcn_sched_barrier(0);            \
    __builtin_amdgcn_s_barrier();                 \
    __builtin_amdgcn_sched_barrier(0);
    issue_x(0);
    if (grp == 1) { issue_w(0, 0); issue_w(1, 0); } else issue_w(0, 1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (LN == 1 && tid < BM) {                     // the partials were requested before the first pieces: no extra wait here
        float ms = 0.f, m2 = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t) { ms += pt[t].mean; m2 += pt[t].m2; }
        const float mean = ms / (float)nst;
        float dev = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t) if (t < nst) { const float d = pt[t].mean - mean; dev += d * d; }
        ln_row = make_float2(mean, rsqrtf((m2 + 256.f * dev) / (float)K + 1e-5f));
    }
    PP_BAR()
    if (grp == 1) { PP_BAR() }
    f16x8 fa[TN], fa2[TN], fb[TM];
    if (TRACE) { tr_t0 = clock64(); tr_w0 = wall_clock64(); }
    for (int j = 0; j < np; ++j) {
        const char* xb = smem + (j & 1) * XBUF;
        const char* wb = smem + WBASE + (j % 3) * WBUF;
        long long c0 = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0;
        if (TRACE) c0 = clock64();
#pragma unroll
        for (int ni = 0; ni < TN; ++ni) fa[ni] = *(const f16x8*)(wb + wo0 + ni * 2048);
#pragma unroll
        for (int mi = 0; mi < TM; ++mi) fb[mi] = *(const f16x8*)(xb + xo0 + mi * 2048);
        if (j + 1 < np) issue_x(j + 1);
        if (grp == 1) { if (j + 2 < np) issue_w(j + 2, 0); }
        else if (j + 1 < np) issue_w(j + 1, 1);
        if (TRACE) c1 = clock64();
        PP_BAR()
        if (TRACE) c2 = clock64();
        __builtin_amdgcn_s_setprio(1);
        // The second k32 sub-step's fragments are read DURING the first sub-step's MFMAs, by inline-asm ds_read_b128 with counted waits
        // (round 4).  Written as plain loads hipcc put `s_waitcnt lgkmcnt(0)` in front of the segment's first MFMA (right behind the four
        // W reads it had just issued: their whole LDS latency exposed) and again in front of the second sub-step (behind the x reload it
        // had issued three MFMAs earlier): MMA segment 1 180 cycles for 1 024 cycles of MFMAs.  Now: MFMA group 0 starts at once (its
        // operands were read in the LOAD segment), the four W reads follow it, the x fragment mi is re-read two groups after its last use
        // (a read into a register an in-flight MFMA still reads stalls the issue), and every group of the second sub-step waits only for
        // the reads it consumes -- LDS returns in order, so `lgkmcnt(n)` with n = the reads issued after them.  The wait names its
        // registers as operands: the MFMAs that consume them cannot be scheduled in front of it (guide 5.4 rule 18).  Same MFMAs on
        // the same operands in the same order: the same numbers.  Interleaved with the compiler-placed form on one box (M = 66 560): in_proj 247.8 vs
        // 258.3 us, c_fc + QuickGELU 327.9 vs 337.0, out_proj 136.3 vs 138.1, c_proj 340.7 vs 348.3; 13.01 vs 13.33 ms of GEMMs per frame.
        const unsigned xa1 = lds0 + (unsigned)((j & 1) * XBUF + xo1), wa1 = lds0 + (unsigned)(WBASE + (j % 3) * WBUF + wo1);
#define PP_DS128(DST, ADDR, OFF) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(DST) : "v"(ADDR), "n"(OFF))
#define PP_GROUP(FA, MI)                                                                                              \
        _Pragma("unroll") for (int ni = 0; ni < TN; ++ni)                                                             \
            acc[ni][MI] = __builtin_amdgcn_mfma_f32_16x16x32_f16(FA[ni], fb[MI], acc[ni][MI], 0, 0, 0);
        PP_GROUP(fa, 0)
        PP_DS128(fa2[0], wa1, 0); PP_DS128(fa2[1], wa1, 2048); PP_DS128(fa2[2], wa1, 4096); PP_DS128(fa2[3], wa1, 6144);
        __builtin_amdgcn_sched_barrier(0);
        PP_GROUP(fa, 1)
        __builtin_amdgcn_sched_barrier(0);
        PP_GROUP(fa, 2) PP_DS128(fb[0], xa1, 0);          __builtin_amdgcn_sched_barrier(0);
        PP_GROUP(fa, 3) PP_DS128(fb[1], xa1, 2048);       __builtin_amdgcn_sched_barrier(0);
        PP_GROUP(fa, 4) PP_DS128(fb[2], xa1, 2 * 2048);   __builtin_amdgcn_sched_barrier(0);
        PP_GROUP(fa, 5) PP_DS128(fb[3], xa1, 3 * 2048);   __builtin_amdgcn_sched_barrier(0);
        PP_GROUP(fa, 6) PP_DS128(fb[4], xa1, 4 * 2048);   __builtin_amdgcn_sched_barrier(0);
        PP_GROUP(fa, 7) PP_DS128(fb[5], xa1, 5 * 2048);   __builtin_amdgcn_sched_barrier(0);
        // reads in flight, oldest first: fa2[0..3], fb[0..5]; fb[6], fb[7] follow groups 0 and 1 of the second sub-step
        asm volatile("s_waitcnt lgkmcnt(5)" : "+v"(fa2[0]), "+v"(fa2[1]), "+v"(fa2[2]), "+v"(fa2[3]), "+v"(fb[0]));
        PP_GROUP(fa2, 0) PP_DS128(fb[6], xa1, 6 * 2048);  __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt lgkmcnt(5)" : "+v"(fb[1]));
        PP_GROUP(fa2, 1) PP_DS128(fb[7], xa1, 7 * 2048);  __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt lgkmcnt(5)" : "+v"(fb[2]));
        PP_GROUP(fa2, 2) __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(fb[3]));
        PP_GROUP(fa2, 3) __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt lgkmcnt(3)" : "+v"(fb[4]));
        PP_GROUP(fa2, 4) __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(fb[5]));
        PP_GROUP(fa2, 5) __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt lgkmcnt(1)" : "+v"(fb[6]));
        PP_GROUP(fa2, 6) __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(fb[7]));
        PP_GROUP(fa2, 7) __builtin_amdgcn_sched_barrier(0);
#undef PP_GROUP
#undef PP_DS128
        __builtin_amdgcn_s_setprio(0);
        if (TRACE) c3 = clock64();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");              // my pieces issued in this phase have landed
        if (TRACE) c4 = clock64();
        PP_BAR()
        if (TRACE) { const long long c5 = clock64(); tr_load += c1 - c0; tr_bar += (c2 - c1) + (c5 - c4); tr_mma += c3 - c2; tr_wait += c4 - c3; }
    }
    if (TRACE) tr_main += clock64() - tr_t0;
    if (grp == 0) { PP_BAR() }
#undef PP_BAR
    // ---- epilogue: the same chunk-XOR-swizzled LDS image as k_gemm_f16_pp ----
    __syncthreads();
    if (EPI == EPI_BIAS || EPI == EPI_BIAS_GELU || EPI == EPI_BIAS_RESID_H) {
        float ln_mean[TM], ln_rstd[TM];
        if (LN == 1) {                      // the tile's 256 (mean, rstd) pairs go through LDS (above the 128 KB output image)
            float2* lsm = (float2*)(smem + 131072);
            if (tid < BM) lsm[tid] = ln_row;
            __syncthreads();
#pragma unroll
            for (int mi = 0; mi < TM; ++mi) {
                const float2 t2 = lsm[grp * 128 + mi * 16 + r15];
                ln_mean[mi] = t2.x; ln_rstd[mi] = t2.y;
            }
        }
#pragma unroll
        for (int ni = 0; ni < TN; ++ni) {
            const int nloc = wn * 64 + ni * 16 + 4 * q4;
            const float4 b4 = *(const float4*)(bias + n0 + nloc);
            float4 c4 = make_float4(0.f, 0.f, 0.f, 0.f);
            if (LN == 1) c4 = *(const float4*)(ln_c1 + n0 + nloc);
            const int ch = nloc >> 3, hf = (nloc >> 2) & 1;
#pragma unroll
            for (int mi = 0; mi < TM; ++mi) {
                const int m = grp * 128 + mi * 16 + r15;
                float v[4] = {acc[ni][mi][0] + b4.x, acc[ni][mi][1] + b4.y, acc[ni][mi][2] + b4.z, acc[ni][mi][3] + b4.w};
                if (LN == 1) {
                    v[0] = ln_rstd[mi] * (acc[ni][mi][0] - ln_mean[mi] * c4.x) + b4.x;
                    v[1] = ln_rstd[mi] * (acc[ni][mi][1] - ln_mean[mi] * c4.y) + b4.y;
                    v[2] = ln_rstd[mi] * (acc[ni][mi][2] - ln_mean[mi] * c4.z) + b4.z;
                    v[3] = ln_rstd[mi] * (acc[ni][mi][3] - ln_mean[mi] * c4.w) + b4.w;
                }
                f16x4 h4;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float x = v[e];
                    if (EPI == EPI_BIAS_GELU) x = x * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(x * QGELU_C));
                    h4[e] = (f16)x;
                }
                *(f16x4*)(smem + m * 512 + ((ch ^ (m & 31)) << 4) + hf * 8) = h4;
            }
        }
        __syncthreads();
        const int j = tid & 31, rr = tid >> 5;
        if (EPI == EPI_BIAS_RESID_H) {
            // fp16 residual stream, updated in place: x = f16(x + f16(acc + bias)) -- the arithmetic of upstream's fp16 run
            // (model.py:190-191 on half tensors).  Eight residual loads go out before the first store.
            f16* xr = (f16*)resid;
#pragma unroll
            for (int p8 = 0; p8 < 2; ++p8) {
                f16x8 x8[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const int m = (p8 * 8 + q) * 16 + rr;
                    x8[q] = *(const f16x8*)(xr + (size_t)(m0 + m) * ldc + n0 + ((j ^ (m & 31)) << 3));
                }
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const int m = (p8 * 8 + q) * 16 + rr;
                    const f16x8 v = *(const f16x8*)(smem + m * 512 + j * 16);
                    f16x8 o;
#pragma unroll
                    for (int e = 0; e < 8; ++e) o[e] = (f16)((float)x8[q][e] + (float)v[e]);
                    *(f16x8*)(xr + (size_t)(m0 + m) * ldc + n0 + ((j ^ (m & 31)) << 3)) = o;
                }
            }
        } else {
#pragma unroll 4
            for (int pass = 0; pass < 16; ++pass) {
                const int m = pass * 16 + rr;
                const f16x8 v = *(const f16x8*)(smem + m * 512 + j * 16);
                *(f16x8*)((f16*)Cout + (size_t)(m0 + m) * ldc + n0 + ((j ^ (m & 31)) << 3)) = v;
            }
        }
    } else {
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            if (half) __syncthreads();
            if (grp == half) {
#pragma unroll
                for (int ni = 0; ni < TN; ++ni) {
                    const int nloc = wn * 64 + ni * 16 + 4 * q4;
                    float4 b4 = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (EPI == EPI_BIAS_RESID) b4 = *(const float4*)(bias + n0 + nloc);
                    const int ch = nloc >> 2;
#pragma unroll
                    for (int mi = 0; mi < TM; ++mi) {
                        const int m = mi * 16 + r15;
                        *(float4*)(smem + m * 1024 + ((ch ^ (m & 31)) << 4)) =
                            make_float4(acc[ni][mi][0] + b4.x, acc[ni][mi][1] + b4.y, acc[ni][mi][2] + b4.z, acc[ni][mi][3] + b4.w);
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
                    const size_t off = SPLITK ? (size_t)blockIdx.x * 65536 + (size_t)(half * 128 + m) * 256 + ((j ^ (m & 31)) << 2)
                                              : (size_t)(m0 + half * 128 + m) * ldc + n0 + ((j ^ (m & 31)) << 2);
                    if (EPI == EPI_BIAS_RESID) {
                        v.x += x4[q].x; v.y += x4[q].y; v.z += x4[q].z; v.w += x4[q].w;
                        *(float4*)(resid + off) = v;
                        if (LN == 2) {
                            // this wave holds the row's 256 columns of the tile: fp16 copy for the next GEMM + the row's partial statistics
                            const f16x4 h4 = {(f16)v.x, (f16)v.y, (f16)v.z, (f16)v.w};
                            *(f16x4*)(ln_x16 + off) = h4;
                            const float mean = row256_sum((v.x + v.y) + (v.z + v.w)) * (1.0f / 256.0f);
                            const float a = v.x - mean, b = v.y - mean, c = v.z - mean, d = v.w - mean;
                            const float m2 = row256_sum((a * a + b * b) + (c * c + d * d));
                            if (j == 0) ln_stats[(size_t)(m0 + half * 128 + m) * (N >> 8) + tn] = LnPartial{mean, m2};
                        }
                    } else {
                        *(float4*)((float*)Cout + off) = v;
                    }
                }
            }
        }
    }
    if (PERSIST) __syncthreads();          // the epilogue's LDS image is read before the next tile's first pieces land
    }
    if (TRACE && (tid & 63) == 0 && trace) {
        long long* o = trace + ((size_t)blockIdx.x * 8 + wave) * 8;
        const long long t2 = clock64();
        o[0] = tr_main; o[1] = tr_wait; o[2] = tr_bar; o[3] = (t2 - tr_entry) - tr_main; o[4] = tr_load; o[5] = tr_mma; o[6] = wave;
        o[7] = wall_clock64() - tr_w0;
        if (wave == 0) {                       // second record (slots of wave 1..): where the tile's non-MFMA time goes and on which CU
            long long* e = trace + (size_t)gridDim.x * 64 + (size_t)blockIdx.x * 8;
            e[0] = tr_w_entry; e[1] = wall_clock64();
            e[2] = ((long long)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32) | (unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 4);
            e[3] = tr_t0 - tr_entry; e[4] = t2 - tr_t0 - tr_main; e[5] = 1;
        }
    }
}


// ---------------------------------------------------------------------------------------------
// k_gemm_f16_w4 (round 6): the same 256 x 256 x 64 macro tile with FOUR waves, one per SIMD, each 128 tokens x 128 features (8 x 8
// MFMA tiles, 256 accumulators in a0..a255), and a K loop that is ONE hand-scheduled assembly block (csrc/gen_gemm_w4.py writes
// gemm_w4_loop.inc: five-slot LDS ring, one barrier per K-tile, every LDS read / DMA piece / wait at a fixed distance between the
// MFMAs).  A third less LDS read traffic per FLOP than 8 waves x 128 x 64, and no compiler between the MFMAs.
//   A operand = token rows, B operand = weight rows; the LDS image of W is ROW-PERMUTED (through the source addresses of its DMA
//   pieces) so that the eight accumulator tiles ni = 0..7 of a lane are consecutive features: lane (r = lane & 15, q = lane >> 4) of
//   tile (ni, mi), register e holds token mi 16 + 4 q + e and
//       fp16 outputs:  feature 8 r + ni                      -> one 16-byte store per (mi, e), sixteen lanes = 256 contiguous bytes
//       fp32 outputs:  feature 64 (ni >> 2) + 4 r + (ni & 3) -> two 16-byte accesses per (mi, e), sixteen lanes = 256 contiguous bytes
//   of the wave's 128 x 128 quadrant (wm, wn).  The epilogue goes straight from the accumulators to global memory: no LDS image, no
//   barrier.  Same MFMA products in the same K order as k_gemm_f16_pp64 => the same accumulator bits (tests/test_gemm.py).
//   Folded LayerNorm: the producer (LN = 2) writes one (mean, M2) partial per row and 128-COLUMN half (this wave's), the consumer
//   (LN = 1) merges K / 128 of them; k_gemm_f16_pp64 keeps one per 256 columns -- a tower uses one kernel family throughout.
#include "gemm_w4_loop.inc"
// register E of the eight accumulator tiles (ni = 0..7, mi = MI), out of the AGPRs the K loop left them in: a[4 (8 ni + MI) + E].  ONE asm
// statement per eight values, and a whole mi block's four statements in a row: inline asm is a scheduling boundary for hipcc, and with one
// statement per value every element's exp -> add -> rcp chain (QuickGELU) or DPP chain (row statistics) sat alone in its region, padded
// with s_nop (469 per tile in the c_fc epilogue).
template <int MI, int E>
__device__ __forceinline__ void w4_acc8(float (&r)[8]) {
    asm volatile("v_accvgpr_read_b32 %0, a[%8]\n\tv_accvgpr_read_b32 %1, a[%9]\n\tv_accvgpr_read_b32 %2, a[%10]\n\tv_accvgpr_read_b32 %3, a[%11]\n\t"
                 "v_accvgpr_read_b32 %4, a[%12]\n\tv_accvgpr_read_b32 %5, a[%13]\n\tv_accvgpr_read_b32 %6, a[%14]\n\tv_accvgpr_read_b32 %7, a[%15]"
                 : "=v"(r[0]), "=v"(r[1]), "=v"(r[2]), "=v"(r[3]), "=v"(r[4]), "=v"(r[5]), "=v"(r[6]), "=v"(r[7])
                 : "n"(4 * (0 * 8 + MI) + E), "n"(4 * (1 * 8 + MI) + E), "n"(4 * (2 * 8 + MI) + E), "n"(4 * (3 * 8 + MI) + E),
                   "n"(4 * (4 * 8 + MI) + E), "n"(4 * (5 * 8 + MI) + E), "n"(4 * (6 * 8 + MI) + E), "n"(4 * (7 * 8 + MI) + E));
}
template <int MI>
__device__ __forceinline__ void w4_acc_block(float (&r)[4][8]) {       // the 4 x 8 values of an mi block (token 4 q + e, eight features)
    w4_acc8<MI, 0>(r[0]); w4_acc8<MI, 1>(r[1]); w4_acc8<MI, 2>(r[2]); w4_acc8<MI, 3>(r[3]);
}
template <int I> struct w4_ic { static constexpr int value = I; };
template <int... Is, typename F>
__device__ __forceinline__ void w4_for_impl(std::integer_sequence<int, Is...>, F&& f) { (f(w4_ic<Is>{}), ...); }
template <int N, typename F>
__device__ __forceinline__ void w4_for(F&& f) { w4_for_impl(std::make_integer_sequence<int, N>{}, f); }
__device__ __forceinline__ float w4_row16_sum(float v) {      // sum over the 16 lanes of a DPP row (the lanes that share lane >> 4), in every lane
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));    // quad_perm [1,0,3,2]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));    // quad_perm [2,3,0,1]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true));   // row_half_mirror
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, true));   // row_mirror
    return v;
}

#define VG_W4_ASM_OF_(V) VG_W4_ASM_##V
#define VG_W4_ASM_OF(V) VG_W4_ASM_OF_(V)
template <int EPI, int LN = 0, int VAR = 0>
__global__ __launch_bounds__(256, 1) void k_gemm_f16_w4(const f16* __restrict__ X, const f16* __restrict__ Wt,
                                                        const float* __restrict__ bias, void* __restrict__ Cout,
                                                        float* __restrict__ resid, int M, int N, int K, int ldc, int cw,
                                                        const float* __restrict__ ln_c1 = nullptr, LnPartial* __restrict__ ln_stats = nullptr,
                                                        f16* __restrict__ ln_x16 = nullptr, long long* __restrict__ trace = nullptr) {
    constexpr int BM = 256, BN = 256;
    constexpr bool F16OUT = EPI == EPI_BIAS || EPI == EPI_BIAS_GELU;
    constexpr bool HL = EPI == EPI_BIAS_RESID_HL;            // the residual stream as an fp16 pair (hi = ln_x16, lo = (f16*)resid)
    constexpr bool L16 = F16OUT || HL;                       // the accumulator-to-feature layout of 16-bit outputs (eight consecutive features per lane)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    [[maybe_unused]] long long tr_entry = 0, tr_asm0 = 0, tr_asm1 = 0;
    [[maybe_unused]] unsigned t_pro = 0, t_loop = 0, t_wait = 0, t_bar = 0, t_end = 0, t_cal = 0;
    if (VAR == VG_W4_TRACE_VAR) tr_entry = clock64();
    const int ntm = M / BM;
    const int wm = wave >> 1, wn = wave & 1;
    // PERSISTENT: one workgroup per CU walks its XCD's contiguous run of tiles (slot s of G / 8 takes tiles s, s + G / 8, ...: at any time
    // the CUs of an XCD work on neighbouring tiles, the chunked order of the one-tile-per-workgroup kernels)
    const int nt_all = ntm * (N / BN);
    const int xq = nt_all >> 3, xr_ = nt_all & 7, xcd = blockIdx.x & 7;
    const int xbase = (xcd < xr_) ? xcd * (xq + 1) : xr_ * (xq + 1) + (xcd - xr_) * xq;
    const int xcnt = xq + (xcd < xr_ ? 1 : 0);
    const int tstride = (int)(gridDim.x >> 3);
    const int per_chunk = ntm * cw;
    // tile t of the launch -> (row tile, column tile): column tiles in chunks of cw that share their row tile's activations in L2.  One
    // division per tile by the launch constant cw, as a multiplication (exact for t < 2^20, cw <= 2^10); the chunk advances incrementally.
    const unsigned inv_cw = (unsigned)((0x100000000ull + (unsigned)cw - 1u) / (unsigned)cw);
    auto tile_of = [&](int chunk, int tc, int& m0_, int& n0_, int& tn_) {
        const int tm = cw == 1 ? tc : (int)(((unsigned long long)(unsigned)tc * inv_cw) >> 32);      // (cw = 1: the reciprocal 2^32 does not fit)
        tn_ = chunk * cw + (tc - tm * cw);
        m0_ = tm * BM; n0_ = tn_ * BN;
    };
    const int np = K / 64;                          // host guarantees K % 64 == 0 and np >= 4
    constexpr int NSTMAX = 8;                       // width <= 1024
    const int nst = K >> 7;
    const unsigned lds0 = __builtin_amdgcn_readfirstlane((unsigned)(unsigned long)(__attribute__((address_space(3))) char*)smem);
    const unsigned rowbs = __builtin_amdgcn_readfirstlane((unsigned)K * 2u), wdst = (unsigned)wave * 8192u, npu = (unsigned)__builtin_amdgcn_readfirstlane(np);
    unsigned ring = 0, first = 1;
    int ti = (int)(blockIdx.x >> 3);
    if (ti >= xcnt) return;
    int m0, n0, tn;
    int t_chunk = (xbase + ti) / per_chunk, t_tc = (xbase + ti) - t_chunk * per_chunk;      // (the one real division: before the tile loop)
    tile_of(t_chunk, t_tc, m0, n0, tn);
    // Per-tile operands of the epilogue (bias, and for the folded LayerNorm's consumer c1 and the K / 128 partial statistics of the
    // rows wm 128 + lane, wm 128 + 64 + lane).  Vector memory operations retire IN ORDER and the compiler cannot see the K loop's DMA
    // pieces: a load it waits for behind the assembly block would wait for every prefetched piece, and one issued behind the epilogue's
    // stores for the stores to drain.  So tile t + 1's operands are REQUESTED in front of tile t's K loop (older than everything tile t
    // issues) and TAKEN behind tile t's stores, where the compiler's own count of younger operations already allows them to be in flight.
    float4 raw_b[2] = {}, raw_c[2] = {};
    LnPartial raw_pt[2][NSTMAX] = {};
    float4 cur_b[2] = {}, cur_c[2] = {};
    float ln_mean2[2] = {0.f, 0.f}, ln_rstd2[2] = {0.f, 0.f};
    auto issue_raw = [&](int m0_, int n0_, int lane_) {
        const int r15k = lane_ & 15;
        if constexpr (L16) {
            const int ncol = n0_ + wn * 128 + r15k * 8;
            raw_b[0] = *(const float4*)(bias + ncol); raw_b[1] = *(const float4*)(bias + ncol + 4);
            if (LN == 1) { raw_c[0] = *(const float4*)(ln_c1 + ncol); raw_c[1] = *(const float4*)(ln_c1 + ncol + 4); }
        } else if (EPI == EPI_BIAS_RESID) {
            const int ncol = n0_ + wn * 128 + r15k * 4;
            raw_b[0] = *(const float4*)(bias + ncol); raw_b[1] = *(const float4*)(bias + ncol + 64);
        }
        if (LN == 1) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const LnPartial* sp = ln_stats + (size_t)(m0_ + wm * 128 + h * 64 + lane_) * nst;
#pragma unroll
                for (int i = 0; i < NSTMAX; ++i) raw_pt[h][i] = sp[i < nst ? i : nst - 1];     // unconditional loads (a branch around a load costs a vmcnt(0)); the extras are zeroed when taken
            }
        }
    };
    auto take_raw = [&]() {
#pragma unroll
        for (int i = 0; i < 2; ++i) {             // (pinned here: the wait for the loads sits at this point of the program)
            asm volatile("" : "+v"(raw_b[i].x), "+v"(raw_b[i].y), "+v"(raw_b[i].z), "+v"(raw_b[i].w));
            if (LN == 1) asm volatile("" : "+v"(raw_c[i].x), "+v"(raw_c[i].y), "+v"(raw_c[i].z), "+v"(raw_c[i].w));
            cur_b[i] = raw_b[i]; cur_c[i] = raw_c[i];
        }
        if (LN == 1) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                float ms = 0.f, m2 = 0.f;
#pragma unroll
                for (int i = 0; i < NSTMAX; ++i) {
                    asm volatile("" : "+v"(raw_pt[h][i].mean), "+v"(raw_pt[h][i].m2));
                    if (i >= nst) raw_pt[h][i] = LnPartial{0.f, 0.f};
                    ms += raw_pt[h][i].mean; m2 += raw_pt[h][i].m2;
                }
                const float mean = ms / (float)nst;
                float dev = 0.f;
#pragma unroll
                for (int i = 0; i < NSTMAX; ++i) if (i < nst) { const float d = raw_pt[h][i].mean - mean; dev += d * d; }
                ln_mean2[h] = mean;
                ln_rstd2[h] = rsqrtf((m2 + 128.f * dev) / (float)K + 1e-5f);
            }
        }
    };
    issue_raw(m0, n0, lane);
    take_raw();
    for (; ti < xcnt; ti += tstride) {
    int m0n = m0, n0n = n0, tnn = tn;               // the next tile, whose first pieces this tile's last K iterations request (none left: this tile again -- the
    if (ti + tstride < xcnt) {                                                   // pieces land in slots nobody reads and are drained before the workgroup ends)
        t_tc += tstride;
        while (t_tc >= per_chunk) { t_tc -= per_chunk; ++t_chunk; }
        tile_of(t_chunk, t_tc, m0n, n0n, tnn);
    }
    int lane_t;                                    // the lane id, produced INSIDE the loop (v_mbcnt on an opaque zero): a loop-invariant lane id is hoisted, kept live
    { unsigned z_; asm volatile("v_mov_b32 %0, 0" : "=v"(z_)); lane_t = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, z_)); }      // across the whole loop and spilled
    issue_raw(m0n, n0n, lane_t);                    // the NEXT tile's bias / LayerNorm operands: older than this tile's stores (see issue_raw)
    {
    // per-lane operands of the K loop, re-derived per tile from the lane id (a dozen integer instructions): kept live across the tile
    // loop they are what the register allocator spills first -- and it reloads spills behind a vmcnt(0), i.e. behind the previous tile's stores
    // DMA piece p of wave w fills LDS rows 64 w + 8 p + (lane >> 3) of a slot, 16-byte chunk slot lane & 7; the source chunk is
    // (lane & 7) ^ ((LDS row >> 1) & 7) = (lane & 7) ^ (lane >> 4) ^ 4 (p & 1).  X: LDS row = tile row.  W: LDS row h 128 + ni 16 + r
    // (h = w >> 1, ni = 4 (w & 1) + (p >> 1), r = 8 (p & 1) + (lane >> 3)) holds the feature the output layout asks for (above).
    const unsigned rowb = (unsigned)K * 2u;
    const int lane = lane_t;
    const unsigned c0 = (unsigned)((lane & 7) ^ (lane >> 4));
    const unsigned dv0 = (unsigned)(lane >> 3) * rowb + (c0 << 4), dv1 = (unsigned)(lane >> 3) * rowb + ((c0 ^ 4u) << 4);
    const unsigned wlm = L16 ? 8u : 4u;                                      // feature step per (lane >> 3)
    const unsigned dw0 = (unsigned)(lane >> 3) * wlm * rowb + (c0 << 4), dw1 = (unsigned)(lane >> 3) * wlm * rowb + ((c0 ^ 4u) << 4);
    const unsigned wpo = __builtin_amdgcn_readfirstlane((L16 ? 64u : 32u) * rowb);        // odd pieces: r += 8
    const int wrow0 = (wave >> 1) * 128 + (L16 ? (wave & 1) * 4 : (wave & 1) * 64);         // feature of (ni = 4 (w & 1), r = 0)
    const int r15t = lane & 15, q4t = lane >> 4;
    const unsigned swz = (unsigned)((r15t >> 1) & 7);
    const unsigned xo0 = (unsigned)(wm * 128 + r15t) * 128u + (((unsigned)q4t ^ swz) << 4), xo1 = (unsigned)(wm * 128 + r15t) * 128u + (((unsigned)(4 + q4t) ^ swz) << 4);
    const unsigned wo0 = (unsigned)(wn * 128 + r15t) * 128u + (((unsigned)q4t ^ swz) << 4), wo1 = (unsigned)(wn * 128 + r15t) * 128u + (((unsigned)(4 + q4t) ^ swz) << 4);
        const unsigned long long xp = (unsigned long long)(X + (size_t)(m0 + wave * 64) * K), xpn = (unsigned long long)(X + (size_t)(m0n + wave * 64) * K);
        const unsigned long long wp = (unsigned long long)(Wt + (size_t)(n0 + wrow0) * K), wpn = (unsigned long long)(Wt + (size_t)(n0n + wrow0) * K);
        const unsigned xlo = __builtin_amdgcn_readfirstlane((unsigned)xp), xhi = __builtin_amdgcn_readfirstlane((unsigned)(xp >> 32));
        const unsigned wlo = __builtin_amdgcn_readfirstlane((unsigned)wp), whi = __builtin_amdgcn_readfirstlane((unsigned)(wp >> 32));
        const unsigned nxlo = __builtin_amdgcn_readfirstlane((unsigned)xpn), nxhi = __builtin_amdgcn_readfirstlane((unsigned)(xpn >> 32));
        const unsigned nwlo = __builtin_amdgcn_readfirstlane((unsigned)wpn), nwhi = __builtin_amdgcn_readfirstlane((unsigned)(wpn >> 32));
        const unsigned firsts = __builtin_amdgcn_readfirstlane(first);
        ring = __builtin_amdgcn_readfirstlane(ring);
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
#define VG_W4_IN [dv0] "v"(dv0), [dv1] "v"(dv1), [dw0] "v"(dw0), [dw1] "v"(dw1), [xo0] "v"(xo0), [xo1] "v"(xo1), [wo0] "v"(wo0),            \
                 [wo1] "v"(wo1), [xlo] "s"(xlo), [xhi] "s"(xhi), [wlo] "s"(wlo), [whi] "s"(whi), [nxlo] "s"(nxlo), [nxhi] "s"(nxhi),        \
                 [nwlo] "s"(nwlo), [nwhi] "s"(nwhi), [rowb] "s"(rowbs), [wpo] "s"(wpo), [lds0] "s"(lds0), [wdst] "s"(wdst), [np] "s"(npu),  \
                 [first] "s"(firsts)
#define VG_W4_RUN(V) asm volatile(VG_W4_ASM_OF(V) : [ring] "+s"(ring) : VG_W4_IN : VG_W4_CLOBBERS)
#define VG_W4_RUN_TRACE(V)                                                                                                            \
        tr_asm0 = clock64();                                                                                                          \
        asm volatile(VG_W4_ASM_OF(V)                                                                                                  \
                     : [ring] "+s"(ring), [t_pro] "=&s"(t_pro), [t_loop] "=&s"(t_loop), [t_wait] "=&s"(t_wait), [t_bar] "=&s"(t_bar),  \
                       [t_end] "=&s"(t_end), [t_cal] "=&s"(t_cal)                                                                      \
                     : VG_W4_IN : VG_W4_CLOBBERS);                                                                                    \
        tr_asm1 = clock64()
        if constexpr (VAR == 0) { if constexpr (F16OUT) { VG_W4_RUN(0H); } else { VG_W4_RUN(0F); } }
#ifdef VG_DEV      // ablations and alternative schedules (gen_gemm_w4.py VARIANTS): development build, VG_GEMM_W4 = 1 + VAR; fp16 outputs only
        VG_W4_DEV_RUNS
#endif
#undef VG_W4_RUN
#undef VG_W4_RUN_TRACE
#undef VG_W4_IN
#pragma clang diagnostic pop
    }
    // ---- epilogue: accumulators -> global memory ----
    // Addresses are a wave-uniform row pointer (SGPR pair) plus ONE per-lane byte offset: 32 row pointers per lane would not leave room
    // for the residual rows in flight.  The lane id is re-derived per tile (mbcnt) behind an opaque asm: nothing of the epilogue's
    // address arithmetic is hoisted out of the tile loop, across the K loop's assembly block.
    int lane_e;
    { unsigned z_; asm volatile("v_mov_b32 %0, 0" : "=v"(z_)); lane_e = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, z_)); }
    const int r15 = lane_e & 15, q4 = lane_e >> 4;
    const int urow = m0 + wm * 128;                         // wave-uniform first row of the quadrant
    if constexpr (F16OUT) {
        const float bb[8] = {cur_b[0].x, cur_b[0].y, cur_b[0].z, cur_b[0].w, cur_b[1].x, cur_b[1].y, cur_b[1].z, cur_b[1].w};
        const float cc[8] = {cur_c[0].x, cur_c[0].y, cur_c[0].z, cur_c[0].w, cur_c[1].x, cur_c[1].y, cur_c[1].z, cur_c[1].w};
        const unsigned loff = ((unsigned)(4 * q4) * (unsigned)ldc + (unsigned)(r15 * 8)) * 2u;
        const char* cbase = (const char*)((f16*)Cout + (size_t)urow * ldc + n0 + wn * 128);
        // folded LayerNorm: the rows' (mean, rstd) are fetched for FOUR mi blocks at a time, 32 ds_bpermute back to back and pinned behind
        // them (fetched row by row inside the loop every pair sat behind its own lgkmcnt wait -- 32 exposed LDS round trips per tile -- and
        // left alone the compiler sinks every pair back in front of its use).  Row mi 16 + 4 q + e of the wave's half sits in lane
        // (row & 63), register set mi >> 2.
        float rmean[4][4], rrstd[4][4];
        auto fetch_rows = [&](int mg) {
#pragma unroll
            for (int mm = 0; mm < 4; ++mm)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int src = (((mg * 4 + mm) * 16 + 4 * q4 + e) & 63) << 2;
                    rmean[mm][e] = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(src, __builtin_bit_cast(int, ln_mean2[mg])));
                    rrstd[mm][e] = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(src, __builtin_bit_cast(int, ln_rstd2[mg])));
                }
#pragma unroll
            for (int mm = 0; mm < 4; ++mm)
#pragma unroll
                for (int e = 0; e < 4; ++e) asm volatile("" : "+v"(rmean[mm][e]), "+v"(rrstd[mm][e]));
        };
        w4_for<8>([&](auto mic) {
            constexpr int mi = decltype(mic)::value;
            if (LN == 1 && (mi & 3) == 0) fetch_rows(mi >> 2);
            float acc[4][8];
            w4_acc_block<mi>(acc);
            w4_for<4>([&](auto ec) {
                constexpr int e = decltype(ec)::value;
                float mean = 0.f, rstd = 1.f;
                if (LN == 1) { mean = rmean[mi & 3][e]; rstd = rrstd[mi & 3][e]; }
                f16x8 h8;
#pragma unroll
                for (int np2 = 0; np2 < 4; ++np2) {      // feature pairs: the non-transcendental steps as packed fp32 operations (same IEEE operations per element)
                    typedef float f32x2 __attribute__((ext_vector_type(2)));
                    const f32x2 a = {acc[e][2 * np2], acc[e][2 * np2 + 1]}, b2 = {bb[2 * np2], bb[2 * np2 + 1]};
                    f32x2 x = a + b2;
                    if (LN == 1) {
                        const f32x2 c2 = {cc[2 * np2], cc[2 * np2 + 1]};
                        x = rstd * (a - mean * c2) + b2;
                    }
                    if (EPI == EPI_BIAS_GELU) {
                        const f32x2 t = x * QGELU_C;
                        const f32x2 d = f32x2{__builtin_amdgcn_exp2f(t.x), __builtin_amdgcn_exp2f(t.y)} + 1.0f;
                        x = x * f32x2{__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y)};
                    }
                    h8[2 * np2] = (f16)x.x; h8[2 * np2 + 1] = (f16)x.y;
                }
                *(f16x8*)(const_cast<char*>(cbase) + (size_t)(mi * 16 + e) * ldc * 2 + loff) = h8;
            });
        });
    } else if constexpr (HL) {
        // The residual stream as an fp16 PAIR, in the 16-bit layout (a lane holds eight consecutive features of a token): x = hi + lo read as
        // two 16-byte rows, v = x + acc + bias, hi' = f16(v), lo' = f16(v - hi') written as two 16-byte rows; hi' IS the next GEMM's operand.
        // The row statistics are those of hi' + lo' (what every later reader reconstructs).
        const float bb[8] = {cur_b[0].x, cur_b[0].y, cur_b[0].z, cur_b[0].w, cur_b[1].x, cur_b[1].y, cur_b[1].z, cur_b[1].w};
        const unsigned loff = ((unsigned)(4 * q4) * (unsigned)ldc + (unsigned)(r15 * 8)) * 2u;
        char* hbase = (char*)(ln_x16 + (size_t)urow * ldc + n0 + wn * 128);
        char* lbase = (char*)((f16*)resid + (size_t)urow * ldc + n0 + wn * 128);
        constexpr int WIN = 3;                               // mi blocks of the stream in flight (a rolling window: 96 registers; four spilled)
        f16x8 xh[WIN][4], xl[WIN][4];
        auto load_block = [&](int mb) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const size_t ro = (size_t)(mb * 16 + e) * ldc * 2 + loff;
                xh[mb % WIN][e] = *(const f16x8*)(hbase + ro);
                xl[mb % WIN][e] = *(const f16x8*)(lbase + ro);
            }
        };
        load_block(0); load_block(1); load_block(2);
        w4_for<8>([&](auto mic) {
            constexpr int mi = decltype(mic)::value;
            float st_mean[4], st_m2[4];
            float acc[4][8];
            w4_acc_block<mi>(acc);
            w4_for<4>([&](auto ec) {
                constexpr int e = decltype(ec)::value;
                const size_t ro = (size_t)(mi * 16 + e) * ldc * 2 + loff;
                const f16x8 ph = xh[mi % WIN][e], pl = xl[mi % WIN][e];
                f16x8 nh, nl;
                float v[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float t = (acc[e][j] + bb[j]) + ((float)ph[j] + (float)pl[j]);
                    nh[j] = (f16)t;
                    nl[j] = (f16)(t - (float)nh[j]);
                    v[j] = (float)nh[j] + (float)nl[j];
                }
                *(f16x8*)(hbase + ro) = nh;
                *(f16x8*)(lbase + ro) = nl;
                const float mean = w4_row16_sum(((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]))) * (1.0f / 128.0f);
                const float a0 = v[0] - mean, a1 = v[1] - mean, a2 = v[2] - mean, a3 = v[3] - mean;
                const float a4 = v[4] - mean, a5 = v[5] - mean, a6 = v[6] - mean, a7 = v[7] - mean;
                st_mean[e] = mean;
                st_m2[e] = w4_row16_sum(((a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3)) + ((a4 * a4 + a5 * a5) + (a6 * a6 + a7 * a7)));
            });
            if (mi + WIN < 8) load_block(mi + WIN);          // (this block's registers are free: the next one of the window is requested)
            const float mean = r15 == 0 ? st_mean[0] : r15 == 1 ? st_mean[1] : r15 == 2 ? st_mean[2] : st_mean[3];
            const float m2 = r15 == 0 ? st_m2[0] : r15 == 1 ? st_m2[1] : r15 == 2 ? st_m2[2] : st_m2[3];
            if (r15 < 4)
                *(LnPartial*)((char*)(ln_stats + (size_t)(urow + mi * 16) * (size_t)(N >> 7) + 2 * tn + wn) + (unsigned)((4 * q4 + r15) * (N >> 7)) * 8u) = LnPartial{mean, m2};
        });
    } else {
        // fp32: lane holds features 64 g + 4 r + j (ni = 4 g + j) of the wave's 128: two float4 per (mi, e)
        const float4 b4[2] = {cur_b[0], cur_b[1]};          // (zero unless EPI_BIAS_RESID)
        const unsigned loff = ((unsigned)(4 * q4) * (unsigned)ldc + (unsigned)(r15 * 4)) * 4u, loffh = loff >> 1;
        char* fbase = (char*)((EPI == EPI_BIAS_RESID ? resid : (float*)Cout) + (size_t)urow * ldc + n0 + wn * 128);
        // residual rows: the 128 fragment registers of the K loop are free now -- the residual of FOUR mi blocks (32 float4) is requested
        // at once, twice; a row's store follows its own loads only
        float4 xr[4][4][2];
        auto load_group = [&](int mg) {
#pragma unroll
            for (int mm = 0; mm < 4; ++mm)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const char* rp = fbase + (size_t)((mg * 4 + mm) * 16 + e) * ldc * 4 + loff;
                    xr[mm][e][0] = *(const float4*)rp;
                    xr[mm][e][1] = *(const float4*)(rp + 256);
                }
        };
        w4_for<8>([&](auto mic) {
            constexpr int mi = decltype(mic)::value;
            if (EPI == EPI_BIAS_RESID && (mi & 3) == 0) load_group(mi >> 2);
            [[maybe_unused]] float st_mean[4], st_m2[4];
            float acc[4][8];
            w4_acc_block<mi>(acc);
            w4_for<4>([&](auto ec) {
                constexpr int e = decltype(ec)::value;
                float4 v[2];
                char* rp = fbase + (size_t)(mi * 16 + e) * ldc * 4 + loff;
                w4_for<2>([&](auto gc) {
                    constexpr int g = decltype(gc)::value;
                    v[g] = make_float4(acc[e][4 * g + 0] + b4[g].x, acc[e][4 * g + 1] + b4[g].y, acc[e][4 * g + 2] + b4[g].z, acc[e][4 * g + 3] + b4[g].w);
                    if (EPI == EPI_BIAS_RESID) { const float4 x = xr[mi & 3][e][g]; v[g].x += x.x; v[g].y += x.y; v[g].z += x.z; v[g].w += x.w; }
                    *(float4*)(rp + 256 * g) = v[g];
                });
                if (EPI == EPI_BIAS_RESID && LN == 2) {
                    // fp16 copy for the next GEMM + this row's statistics over the wave's 128 columns (every lane of the row's 16 holds them)
                    char* hp = (char*)(ln_x16 + (size_t)(urow + mi * 16 + e) * ldc + n0 + wn * 128) + loffh;
                    const f16x4 h0 = {(f16)v[0].x, (f16)v[0].y, (f16)v[0].z, (f16)v[0].w}, h1 = {(f16)v[1].x, (f16)v[1].y, (f16)v[1].z, (f16)v[1].w};
                    *(f16x4*)hp = h0; *(f16x4*)(hp + 128) = h1;
                    const float mean = w4_row16_sum(((v[0].x + v[0].y) + (v[0].z + v[0].w)) + ((v[1].x + v[1].y) + (v[1].z + v[1].w))) * (1.0f / 128.0f);
                    const float a0 = v[0].x - mean, a1 = v[0].y - mean, a2 = v[0].z - mean, a3 = v[0].w - mean;
                    const float a4 = v[1].x - mean, a5 = v[1].y - mean, a6 = v[1].z - mean, a7 = v[1].w - mean;
                    st_mean[e] = mean;
                    st_m2[e] = w4_row16_sum(((a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3)) + ((a4 * a4 + a5 * a5) + (a6 * a6 + a7 * a7)));
                }
            });
            if (EPI == EPI_BIAS_RESID && LN == 2) {
                // ONE predicated store per mi block, behind the four rows' arithmetic (a branch per row cut the block into four scheduling
                // regions and left every row's DPP chain alone with its s_nops): lane r = e of each 16 writes row e's pair
                const float mean = r15 == 0 ? st_mean[0] : r15 == 1 ? st_mean[1] : r15 == 2 ? st_mean[2] : st_mean[3];
                const float m2 = r15 == 0 ? st_m2[0] : r15 == 1 ? st_m2[1] : r15 == 2 ? st_m2[2] : st_m2[3];
                if (r15 < 4)
                    *(LnPartial*)((char*)(ln_stats + (size_t)(urow + mi * 16) * (size_t)(N >> 7) + 2 * tn + wn) + (unsigned)((4 * q4 + r15) * (N >> 7)) * 8u) = LnPartial{mean, m2};
            }
        });
    }
#ifdef VG_DEV
    if (VAR == VG_W4_TRACE_VAR && lane == 0 && trace) {      // per tile and wave: cycles of entry -> asm, block entry, K loop, its waits, the epilogue
        long long* o = trace + ((size_t)(xbase + ti) * 4 + wave) * 12;
        const long long t2 = clock64();
        o[0] = tr_asm0 - tr_entry; o[1] = t_pro; o[2] = t_loop; o[3] = t_wait; o[4] = t_bar; o[5] = t_end; o[6] = t_cal;
        o[7] = t2 - tr_asm1; o[8] = tr_asm1 - tr_asm0; o[9] = first; o[10] = wave; o[11] = wall_clock64();
        tr_entry = clock64();
    }
#endif
    take_raw();
    m0 = m0n; n0 = n0n; tn = tnn; first = 0;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // the last block's pieces for a "next tile" have landed before the LDS is given back
}

// ---------------------------------------------------------------------------------------------
// Split-K tail of the residual GEMMs (out_proj, c_proj: N = width = three 256-wide column tiles for ViT-B).  One workgroup owns a CU, so a
// launch runs in ROUNDS of n_cu tiles: 333 crops are 257 row tiles x 3 = 771 tiles = three full rounds and a fourth with 3 tiles on 256
// CUs -- the launch takes 4 / 3 of the time for 0.4 % more work (tools/exp_tile_tail.py: +7.6 % tower time from 332 to 333 crops, one
// encode at a time).  The row tiles that do not fill complete rounds are therefore computed K-split: P workgroups per tile, each a
// slice of the K-tiles (k_gemm_f16_pp64<EPI_NONE_F32, ..., SPLITK>: raw fp32 partial tiles into scratch), and k_splitk_resid adds the P
// partials IN FIXED ORDER and applies the residual epilogue -- bias, fp32 residual read-modify-write, and for LN = 2 the fp16 copy and
// the row's partial statistics, the same expressions as the GEMM's own epilogue.  Deterministic; a row in the tail differs from the
// unsplit result by the rounding of ((p0 + p1) + ...) against one fp32 accumulation chain (<= a few 1e-7 relative, tests/test_gemm.py).
template <int LN>
__global__ __launch_bounds__(256) void k_splitk_resid(const float* __restrict__ part, int P, const float* __restrict__ bias,
                                                      float* __restrict__ resid, int N, int ldc, int row0, int ntn,
                                                      LnPartial* __restrict__ ln_stats, f16* __restrict__ ln_x16) {
    // grid: tail tiles x 16; a wave = one row of the tile's 256 columns at a time (lane j: columns 4 j .. 4 j + 3), four rows per wave
    const int tile = blockIdx.x >> 4, rb = blockIdx.x & 15, w = threadIdx.x >> 6, j = threadIdx.x & 63;
    const int tm = tile / ntn, tn = tile - tm * ntn;
    const float4 b4 = *(const float4*)(bias + tn * 256 + 4 * j);
    const float* pb = part + (size_t)tile * P * 65536 + 4 * j;
    float4 x4[4], v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = rb * 16 + w * 4 + i;
        x4[i] = *(const float4*)(resid + (size_t)(row0 + tm * 256 + r) * ldc + tn * 256 + 4 * j);
        v[i] = *(const float4*)(pb + (size_t)r * 256);
    }
    for (int p = 1; p < P; ++p) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = rb * 16 + w * 4 + i;
            const float4 a = *(const float4*)(pb + (size_t)p * 65536 + (size_t)r * 256);
            v[i].x += a.x; v[i].y += a.y; v[i].z += a.z; v[i].w += a.w;
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = rb * 16 + w * 4 + i;
        const size_t off = (size_t)(row0 + tm * 256 + r) * ldc + tn * 256 + 4 * j;
        float4 o = make_float4(v[i].x + b4.x, v[i].y + b4.y, v[i].z + b4.z, v[i].w + b4.w);
        o.x += x4[i].x; o.y += x4[i].y; o.z += x4[i].z; o.w += x4[i].w;
        *(float4*)(resid + off) = o;
        if (LN == 2) {
            const f16x4 h4 = {(f16)o.x, (f16)o.y, (f16)o.z, (f16)o.w};
            *(f16x4*)(ln_x16 + off) = h4;
            const float mean = row256_sum((o.x + o.y) + (o.z + o.w)) * (1.0f / 256.0f);
            const float a = o.x - mean, b = o.y - mean, c = o.z - mean, d = o.w - mean;
            const float m2 = row256_sum((a * a + b * b) + (c * c + d * d));
            if (j == 0) ln_stats[(size_t)(row0 + tm * 256 + r) * (N >> 8) + tn] = LnPartial{mean, m2};
        }
    }
}
