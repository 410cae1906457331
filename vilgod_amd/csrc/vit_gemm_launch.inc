// Part of vit.hip (included in place): how a projection GEMM is launched.  Tile-order and split-K arithmetic, gemm_family (the one
// place a kernel is chosen), one launcher per 256 x 256 kernel and launch_gemm (the one launch path).

// column tiles per L2 chunk: the largest divisor-friendly count whose weight rows (128*K fp16 each) fit ~2.4 MB
static int gemm_chunk_tiles(int N, int K) {
    const int ntn = N / GBN;
    const long tile_bytes = (long)GBN * K * 2;
    int cw_max = (int)(2400000L / tile_bytes);
    if (cw_max < 1) cw_max = 1;
    if (cw_max >= ntn) return ntn;
    int nchunks = (ntn + cw_max - 1) / cw_max;
    while (ntn % nchunks) ++nchunks;
    return ntn / nchunks;
}

// Column tiles (256 wide) per L2 chunk of the tile order for the 256 x 256 kernels.  Measured at M = 64512 (sweep with
// VG_GEMM_CW): sharing one activation row-tile between ALL column tiles that run together wins as long as there are at most
// 9 of them (in_proj 9: 278 vs 292 us; c_proj 3, K = 3072: 302 vs 345 us although its 4.7 MB of weights exceed one XCD's L2 --
// with single-column chunks the 396 MB of hidden activations stream from HBM three times); c_fc (12) is best with 4.
static int gemm_chunk_tiles_256(int ntn) {
    if (ntn <= 9) return ntn;
    int cw = 4;
    while (ntn % cw) --cw;
    return cw;
}

// how a residual GEMM of ntm x ntn tiles is divided: row tiles [0, r_main) in complete rounds, the rest K-split `parts` ways (0 = no split)
struct SplitPlan { int r_main, parts; };
static SplitPlan splitk_plan(int ntm, int ntn, int np, size_t scratch_bytes, int max_parts, int n_cu) {
    // OPT-IN (VG_GEMM_SPLITK=n, read when the handle is made: at most n parts per tile, 8 is the measured optimum; unset / 0 = never split).
    // Measured (tools/bench_gemm_splitk.py, N = 768, one launch at a time): K = 3072 (c_proj) 356 -> 305 us for 3-15 tail tiles, -12 % at 48,
    // -8 % at 72, -2 % at 126; K = 768 (out_proj: the fourth round costs 16 us, two more launches cost as much) -3 % at 6 tiles, +2 % at 30,
    // +9 % at 48: only long K loops are split.  Whole tower (tools/exp_tile_tail.py): one encode at a time 14.12 -> 13.73 ms at 333 crops,
    // 14.35 -> 13.94 at 338; TWO encodes in flight (what the pipeline runs) 12.94 -> 13.01 / 13.27 -> 13.29: the other encode's tiles
    // already fill the last round, and the partial tiles are 60 MB of extra traffic per launch; pipeline 65.5 vs 65.7 frames/s.  So the
    // split is for one-frame-at-a-time (latency) use and stays off in the throughput configuration.
    if (max_parts < 2 || n_cu < 8) return {ntm, 0};        // (more parts = more partial-sum traffic than K-loop saved: 256 KB per part and tile)
    if (np < 24) return {ntm, 0};
    const int total = ntm * ntn, full = total / n_cu;
    if (full < 1) return {ntm, 0};
    const int r_main = full * n_cu / ntn, tail = (ntm - r_main) * ntn;
    if (tail <= 0 || 2 * tail > n_cu) return {ntm, 0};     // a last round that is more than half full is left alone
    int parts = n_cu / tail;
    if (parts > np / 2) parts = np / 2;                    // the kernel's ring needs two K-tiles per workgroup
    if (parts > max_parts) parts = max_parts;
    while (parts >= 2 && (size_t)tail * parts * 262144 > scratch_bytes) --parts;
    if (parts < 2) return {ntm, 0};
    return {r_main, parts};
}

// Which kernel a projection GEMM runs on: the ONE place the choice is made (launch_gemm asks it and launches; vg_gemm_family hands
// the answer to the tests).  fp16, top to bottom: the two fp16-stream epilogues (one kernel family each), then for the ViT shapes
// (gemm_tile256: N % 256 == 0, K >= 128) k_gemm_f16_w4 from four K-tiles up, else k_gemm_f16_pp64; k_gemm_f16 serves the remaining
// legal shapes.  fp32: the MFMA kernel where its tile divides the shape, else the vector-ALU kernel.  Negative: no kernel takes the
// shape (VG_ERR_ARG).  Host arithmetic only.  (The split-K tail of a k_gemm_f16_pp64 launch is launch_gemm's own: it needs the CU count.)
enum { GF_F16 = 0, GF_PP64 = 1, GF_W4 = 2, GF_F32 = 3, GF_F32_MFMA = 4, GF_REFUSED = -1 };
static bool gemm_tile256(int dtype, int N, int K) { return dtype == 1 && N % 256 == 0 && K % 64 == 0 && K / 64 >= 2; }
static int gemm_family(int dtype, int epi, int M, int N, int K, int gemm_w4, bool f32_mfma, bool use_pp) {
    const bool w4 = gemm_w4 && K / 64 >= 4;        // (k_gemm_f16_w4's ring wants four K-tiles)
    if (epi == EPI_BIAS_RESID_HL)                  // the stream as an fp16 pair: k_gemm_f16_w4's producer epilogue only
        return use_pp && w4 && M % 256 == 0 ? GF_W4 : GF_REFUSED;
    if (epi == EPI_BIAS_RESID_H)                   // fp16 residual stream: only k_gemm_f16_pp64 implements it
        return use_pp && M % 256 == 0 ? GF_PP64 : GF_REFUSED;
    if (epi < EPI_BIAS || epi > EPI_NONE_F32) return GF_REFUSED;
    if (dtype == 1) {
        if (M % GBM || N % GBN || K % GK) return GF_REFUSED;
        if (use_pp) return w4 ? GF_W4 : GF_PP64;
        return GF_F16;
    }
    if (M % 64 || N % 64 || K % 16) return GF_REFUSED;
    return M % 128 == 0 && N % 128 == 0 && f32_mfma ? GF_F32_MFMA : GF_F32;     // (VG_GEMM_F32_MFMA=0: the vector-ALU kernel for every shape, bit-identical)
}

#ifdef VG_DEV      // dev_tile_order
#include "dev/vit_dev_tile_order.inc"
#endif

// column tiles per L2 chunk of a launch of family `fam` (GF_F16, GF_PP64, GF_W4); *cap: the persistent grid's workgroups
static int gemm_tile_chunk(int fam, int N, int K, int* cap = nullptr) {
    int cwt = fam == GF_F16 ? gemm_chunk_tiles(N, K) : gemm_chunk_tiles_256(N / 256);
#ifdef VG_DEV      // tile-order sweeps and the half-grid experiment (VG_GEMM_NO_CHUNK, VG_GEMM_CW, VG_GEMM_W4_GRID)
    dev_tile_order(fam, N, &cwt, cap);
#endif
    return cwt;
}

template <int EPI, bool TRACE = false, bool PERSIST = false, int LN = 0>
static int launch_gemm_pp64(const void* X, const void* Wt, const float* bias, void* C, float* resid, int M, int N, int K, int ldc,
                            hipStream_t st, long long* trace = nullptr, const float* ln_c1 = nullptr, LnPartial* ln_stats = nullptr,
                            f16* ln_x16 = nullptr) {
    if (M % 256 || N % 256 || K % 64 || K / 64 < 2) return VG_ERR_ARG;
    if (LN == 1 && (K % 256 || K > 1024 || !ln_c1 || !ln_stats)) return VG_ERR_ARG;      // the consumer merges at most 4 partials (pt[4])
    if (LN == 2 && (ldc != N || !ln_stats || !ln_x16)) return VG_ERR_ARG;
    auto kern = k_gemm_f16_pp64<EPI, TRACE, PERSIST, LN>;
    const int lds = 5 * 32768;
    VG_MAX_DYNAMIC_LDS(kern, lds);
    const int ntn = N / 256, cwt = gemm_tile_chunk(GF_PP64, N, K);
    int grid = (M / 256) * ntn;
    if (PERSIST) grid = vg_persistent_grid(grid, vg_cu_count());
    hipLaunchKernelGGL(kern, dim3(grid), dim3(512), lds, st, (const f16*)X, (const f16*)Wt, bias, C, resid, M, N, K,
                       ldc, cwt, trace, ln_c1, ln_stats, ln_x16, 1);
    VG_LAUNCH_CHECK();
    return VG_OK;
}

template <int EPI, int LN = 0, int VAR = 0>
static int launch_gemm_w4(const void* X, const void* Wt, const float* bias, void* C, float* resid, int M, int N, int K, int ldc,
                          hipStream_t st, const float* ln_c1 = nullptr, LnPartial* ln_stats = nullptr, f16* ln_x16 = nullptr,
                          long long* trace = nullptr) {
    if (M % 256 || N % 256 || K % 64 || K / 64 < 4) return VG_ERR_ARG;
    if (LN == 1 && (K % 128 || K > 1024 || !ln_c1 || !ln_stats)) return VG_ERR_ARG;
    if (LN == 2 && (ldc != N || !ln_stats || !ln_x16)) return VG_ERR_ARG;
    auto kern = k_gemm_f16_w4<EPI, LN, VAR>;
    const int lds = 5 * 32768;
    VG_MAX_DYNAMIC_LDS(kern, lds);
    const int ntn = N / 256;
    int cap = vg_cu_count();                         // persistent grid: one workgroup per CU
    const int cwt = gemm_tile_chunk(GF_W4, N, K, &cap);
    const int grid = vg_persistent_grid((M / 256) * ntn, cap);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, st, (const f16*)X, (const f16*)Wt, bias, C, resid, M, N, K,
                       ldc, cwt, ln_c1, ln_stats, ln_x16, trace);
    VG_LAUNCH_CHECK();
    return VG_OK;
}

// rows [row0, row0 + Mt) of a residual GEMM, K-split `parts` ways through `scratch` (see k_splitk_resid)
template <int LN>
static int launch_gemm_resid_tail(const void* X, const void* Wt, const float* bias, float* resid, int row0, int Mt, int N, int K, int ldc,
                                  int parts, float* scratch, hipStream_t st, LnPartial* ln_stats, f16* ln_x16) {
    if (Mt % 256 || N % 256 || K % 64 || parts < 2 || K / 64 / parts < 2 || !scratch) return VG_ERR_ARG;
    auto kern = k_gemm_f16_pp64<EPI_NONE_F32, false, false, 0, true>;
    const int lds = 5 * 32768;
    VG_MAX_DYNAMIC_LDS(kern, lds);
    const int ntn = N / 256, tiles = (Mt / 256) * ntn;
    hipLaunchKernelGGL(kern, dim3(tiles * parts), dim3(512), lds, st, (const f16*)X + (size_t)row0 * K, (const f16*)Wt, (const float*)nullptr,
                       (void*)scratch, (float*)nullptr, Mt, N, K, 256, ntn, (long long*)nullptr, (const float*)nullptr, (LnPartial*)nullptr,
                       (f16*)nullptr, parts);
    VG_LAUNCH_CHECK();
    hipLaunchKernelGGL((k_splitk_resid<LN>), dim3(tiles * 16), dim3(256), 0, st, (const float*)scratch, parts, bias, resid, N, ldc, row0, ntn,
                       ln_stats, ln_x16);
    VG_LAUNCH_CHECK();
    return VG_OK;
}

#ifdef VG_DEV      // the superseded kernels (K-step-32 ping-pong, k_gemm_f16_x2), their launchers and dev_launch_gemm
#include "dev/vit_dev_launchers.inc"
#endif

// Every projection GEMM of the tower and of the test entry points: the kernel gemm_family names, and for the residual GEMMs of the
// k_gemm_f16_pp64 family the split-K tail where scratch is at hand.
template <int EPI, int LN = 0>
static int launch_gemm(const GemmCfg& g, GemmProfile* pr, const void* X, const void* Wt, const float* bias, void* C, float* resid, int M,
                       int N, int K, hipStream_t st, int ldc = 0, const float* ln_c1 = nullptr, LnPartial* ln_stats = nullptr,
                       f16* ln_x16 = nullptr, float* sk_scratch = nullptr, size_t sk_bytes = 0) {
    if (ldc == 0) ldc = N;
    bool use_pp = gemm_tile256(g.dtype, N, K);
    struct Closer {                                // the profiling sample ends wherever the launch returns
        GemmProfile* pr; hipStream_t st; double fl; int kind;
        ~Closer() { if (pr) pr->end(st, kind, fl); }
    } closer{pr && pr->begin(st) ? pr : nullptr, st, 2.0 * (double)M * (double)N * (double)K, use_pp ? 1 : 0};
#ifdef VG_DEV      // the development build's experiments (dev/vit_dev_launchers.inc) may take the launch over or send it to k_gemm_f16
    { const int rc = dev_launch_gemm<EPI, LN>(g, X, Wt, bias, C, resid, M, N, K, st, ldc, ln_c1, ln_stats, ln_x16, &use_pp); if (rc != VG_DEV_PASS) return rc; }
    closer.kind = use_pp ? 1 : 0;
#endif
    const int fam = gemm_family(g.dtype, EPI, M, N, K, g.gemm_w4, g.f32_mfma, use_pp);
    if (fam < 0) return VG_ERR_ARG;
    if constexpr (EPI == EPI_BIAS_RESID_HL) {
        if (!(LN == 2 && resid && ln_x16)) return VG_ERR_ARG;
        return launch_gemm_w4<EPI, LN>(X, Wt, bias, C, resid, M, N, K, ldc, st, ln_c1, ln_stats, ln_x16);
    } else if constexpr (EPI == EPI_BIAS_RESID_H) {
        return launch_gemm_pp64<EPI>(X, Wt, bias, C, resid, M, N, K, ldc, st);
    } else if (fam == GF_W4) {
        return launch_gemm_w4<EPI, LN>(X, Wt, bias, C, resid, M, N, K, ldc, st, ln_c1, ln_stats, ln_x16);
    } else if (fam == GF_PP64) {
        if constexpr (EPI == EPI_BIAS_RESID && LN != 1) {
            // residual GEMMs with scratch at hand: the row tiles beyond the last complete round of tiles run K-split
            // (not k_gemm_f16_w4's: persistent workgroups have no tile rounds to fill)
            if (sk_scratch && M % 256 == 0) {
                const SplitPlan sp = splitk_plan(M / 256, N / 256, K / 64, sk_bytes, g.splitk_max, vg_cu_count());
                if (sp.parts) {
                    const int rc = launch_gemm_pp64<EPI, false, false, LN>(X, Wt, bias, C, resid, sp.r_main * 256, N, K, ldc, st, nullptr, ln_c1, ln_stats, ln_x16);
                    if (rc) return rc;
                    return launch_gemm_resid_tail<LN>(X, Wt, bias, resid, sp.r_main * 256, M - sp.r_main * 256, N, K, ldc, sp.parts, sk_scratch, st,
                                                      ln_stats, ln_x16);
                }
            }
        }
        return launch_gemm_pp64<EPI, false, false, LN>(X, Wt, bias, C, resid, M, N, K, ldc, st, nullptr, ln_c1, ln_stats, ln_x16);
    } else if (fam == GF_F16) {
        if (LN != 0) return VG_ERR_ARG;            // the folded LayerNorm exists in the 256 x 256 kernels only
        VG_MAX_DYNAMIC_LDS(k_gemm_f16<EPI>, G_LDS_BYTES);
        hipLaunchKernelGGL((k_gemm_f16<EPI>), dim3((M / GBM) * (N / GBN)), dim3(512), G_LDS_BYTES, st, (const f16*)X, (const f16*)Wt, bias, C,
                           resid, M, N, K, ldc, gemm_tile_chunk(GF_F16, N, K));
    } else if (fam == GF_F32_MFMA) {
        hipLaunchKernelGGL((k_gemm_f32_mfma<EPI>), dim3((M / 128) * (N / 128)), dim3(256), 0, st, (const float*)X, (const float*)Wt, bias,
                           (float*)C, resid, M, N, K);
    } else {
        hipLaunchKernelGGL((k_gemm_f32<EPI>), dim3((M / 64) * (N / 64)), dim3(256), 0, st, (const float*)X, (const float*)Wt, bias,
                           (float*)C, resid, M, N, K);
    }
    VG_LAUNCH_CHECK();
    return VG_OK;
}
