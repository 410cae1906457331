// Development build only (-DVG_DEV, libvilgod_hip_dev.so): included by ../vit_gemm_launch.inc in place.
// The superseded kernels: the K-step-32 ping-pong kernels (kept for the cycle-stamp tools) and k_gemm_f16_x2 (measured slower than
// k_gemm_f16_pp64 on every projection shape, LAB_NOTES.md section 3, round 3; VG_GEMM_X2=1); then their launchers and dev_launch_gemm.
#include "vit_gemm_pp32.inc"
#include "vit_gemm_pp16.inc"
#include "vit_gemm_x2.inc"

template <int EPI, int STAGES>
static int launch_gemm_pp16(const void* X, const void* Wt, const float* bias, void* C, float* resid, int M, int N, int K, int ldc,
                            hipStream_t st) {
    if (M % 256 || N % 256 || K % GK || K / GK < STAGES) return VG_ERR_ARG;
    auto kern = k_gemm_f16_pp16<EPI, STAGES>;
    const int lds = STAGES * 32768;
    VG_MAX_DYNAMIC_LDS(kern, lds);
    const int ntn = N / 256;
    int cwt = gemm_chunk_tiles_256(ntn);
    hipLaunchKernelGGL(kern, dim3((M / 256) * ntn), dim3(512), lds, st, (const f16*)X, (const f16*)Wt, bias, C, resid, M, N, K,
                       ldc, cwt);
    VG_LAUNCH_CHECK();
    return VG_OK;
}

template <int EPI, int STAGES, bool TRACE, int PH = 2>
static int launch_gemm_pp(const void* X, const void* Wt, const float* bias, void* C, float* resid, int M, int N, int K, int ldc,
                          hipStream_t st, long long* trace) {
    if (M % 256 || N % 256 || K % GK || K / GK < STAGES) return VG_ERR_ARG;
    auto kern = k_gemm_f16_pp<EPI, STAGES, TRACE, PH>;
    const int lds = STAGES * 32768;
    VG_MAX_DYNAMIC_LDS(kern, lds);
    const int ntn = N / 256;
    int cwt = gemm_chunk_tiles_256(ntn);
    hipLaunchKernelGGL(kern, dim3((M / 256) * ntn), dim3(512), lds, st, (const f16*)X, (const f16*)Wt, bias, C, resid, M, N, K,
                       ldc, cwt, trace);
    VG_LAUNCH_CHECK();
    return VG_OK;
}

// The experiments of the development build inside launch_gemm, called at one point (after the profiling pair is open, before the product
// dispatch).  Returns the result of the launch it ran (or refused) itself, VG_DEV_PASS when the product dispatch is to go on.  May clear
// *use_pp to send every shape to k_gemm_f16.
#define VG_DEV_PASS (-1000)
template <int EPI, int LN>
static int dev_launch_gemm(const GemmCfg& g, const void* X, const void* Wt, const float* bias, void* C, float* resid, int M, int N, int K,
                            hipStream_t st, int ldc, const float* ln_c1, LnPartial* ln_stats, f16* ln_x16, bool* use_pp) {
    if (getenv("VG_GEMM_V4")) *use_pp = false;          // every shape through k_gemm_f16 (tools/dev/bench_gemm_v4.sh)
    if constexpr (EPI == EPI_BIAS_RESID_HL || EPI == EPI_BIAS_RESID_H) return VG_DEV_PASS;
    else {
        if (g.dtype != 1 || !*use_pp || M % GBM || N % GBN || K % GK) return VG_DEV_PASS;
        // persistent workgroups (one per CU walking its XCD's run of tiles) per epilogue kind, bit EPI of VG_GEMM_PERSIST.  Alone at
        // M = 64256: in_proj (+bias) 271 -> 244 us, c_fc (GELU) and out_proj +-0, c_proj -3 %; inside the pipeline no measurable change
        // (13.65-13.70 ms of GEMMs per frame either way): the next tile's first pieces still wait for the previous tile's stores (one
        // vmcnt), so only the dispatch gap is saved.
        static const int persist_mask = getenv("VG_GEMM_PERSIST") ? atoi(getenv("VG_GEMM_PERSIST")) : 0;
        if constexpr (LN == 0 && (EPI == EPI_BIAS || EPI == EPI_BIAS_GELU || EPI == EPI_BIAS_RESID)) {
            if ((persist_mask >> EPI) & 1) return launch_gemm_pp64<EPI, false, true>(X, Wt, bias, C, resid, M, N, K, ldc, st);
        }
        if (g.gemm_x2 && K % 256 == 0 && (LN != 1 || K / 64 <= X2_LN_MAXP))
            return launch_gemm_x2<EPI, LN>(X, Wt, bias, C, resid, M, N, K, ldc, st, ln_c1, ln_stats, ln_x16);
        if (g.gemm_x2 && LN != 0) return VG_ERR_ARG;       // (the two kernels keep different partial statistics)
        if constexpr (LN == 0 && EPI == EPI_BIAS) {        // k_gemm_f16_w4's ablations and alternative schedules: VG_GEMM_W4 = 1 + VAR
            if (g.gemm_w4 && K / 64 >= 4) switch (g.gemm_w4) { VG_W4_DEV_CASES(EPI, LN) }
        }
        return VG_DEV_PASS;
    }
}
