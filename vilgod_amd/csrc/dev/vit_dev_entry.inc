// Development build only (-DVG_DEV, libvilgod_hip_dev.so): included by ../vit.hip in place.  vg_vit_create's hook and the development
// aids of tools/dev/vilgod_hip_dev.h: ablations, cycle-stamp traces.

// called by vg_vit_create once the tower's switches are resolved
static void dev_vit_create(vg_vit* v) {
    const bool v4 = getenv("VG_GEMM_V4") != nullptr;
    if (v4) v->resid_h = v->ln_fold = false;      // (k_gemm_f16 has neither epilogue)
    // k_gemm_f16_x2 serves K % 256 == 0 and merges at most X2_LN_MAXP partial statistics per row: a tower uses it for all of its
    // projection GEMMs or for none (the two kernels keep the folded LayerNorm's partials at different granularity)
    v->gemm.gemm_x2 = env_on("VG_GEMM_X2", false) && v->dtype == 1 && v->width % 256 == 0 && v->width / 64 <= X2_LN_MAXP && !v->resid_h && !v4;
}

extern "C" {

/* ablation variants of the f16 GEMMs (development aid, epi 0 only): k_gemm_f16 var 0 = as shipped, 1 = no DMA inside the
 * K loop, 2 = DMA only (no LDS reads / MFMA), 3 = no epilogue; k_gemm_f16_pp var 22 = as shipped (4 stages, one phase per
 * K-step), 20 = two phases per K-step, 21 / 23 = 5 stages */
int vg_gemm_variant(int var, const void* d_X, const void* d_Wt, const float* d_bias, void* d_C, int M, int N, int K, int ldc, void* stream) {
    if (M % GBM || N % GBN || K % GK) return VG_ERR_ARG;
    int nwg = (M / GBM) * (N / GBN);
    hipStream_t st = (hipStream_t)stream;
#define VG_VAR(V)                                                                                                          \
    case V:                                                                                                                \
        (void)hipFuncSetAttribute((const void*)k_gemm_f16<EPI_BIAS, V>, hipFuncAttributeMaxDynamicSharedMemorySize, G_LDS_BYTES); \
        hipLaunchKernelGGL((k_gemm_f16<EPI_BIAS, V>), dim3(nwg), dim3(512), G_LDS_BYTES, st, (const f16*)d_X, (const f16*)d_Wt, \
                           d_bias, d_C, nullptr, M, N, K, ldc, gemm_tile_chunk(GF_F16, N, K));                            \
        break;
    switch (var) { VG_VAR(0) VG_VAR(1) VG_VAR(2) VG_VAR(3)
        case 20: return launch_gemm_pp<EPI_BIAS, 4, false>(d_X, d_Wt, d_bias, d_C, nullptr, M, N, K, ldc, st, nullptr);
        case 21: return launch_gemm_pp<EPI_BIAS, 5, false>(d_X, d_Wt, d_bias, d_C, nullptr, M, N, K, ldc, st, nullptr);
        case 22: return launch_gemm_pp<EPI_BIAS, 4, false, 1>(d_X, d_Wt, d_bias, d_C, nullptr, M, N, K, ldc, st, nullptr);
        case 23: return launch_gemm_pp<EPI_BIAS, 5, false, 1>(d_X, d_Wt, d_bias, d_C, nullptr, M, N, K, ldc, st, nullptr);
        case 30: return launch_gemm_pp16<EPI_BIAS, 4>(d_X, d_Wt, d_bias, d_C, nullptr, M, N, K, ldc, st);
        case 32: return launch_gemm_pp64<EPI_BIAS>(d_X, d_Wt, d_bias, d_C, nullptr, M, N, K, ldc, st);
        case 36: return launch_gemm_pp64<EPI_BIAS, false, true>(d_X, d_Wt, d_bias, d_C, nullptr, M, N, K, ldc, st);
        default: return VG_ERR_ARG; }
#undef VG_VAR
    VG_LAUNCH_CHECK();
    return VG_OK;
}

/* k_gemm_f16_pp64 with the folded LayerNorm's CONSUMER epilogue (LN = 1; epi 0 bias, 1 bias + QuickGELU) on caller-supplied row
 * statistics: d_stats [M, K/256] (mean, m2) pairs, d_c1 [N]; for A/B runs against vg_gemm on the same operands */
int vg_gemm_ln_consumer(int epi, const void* d_X, const void* d_Wt, const float* d_bias, const float* d_c1, const void* d_stats,
                        void* d_C, int M, int N, int K, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (epi == 0) return launch_gemm_pp64<EPI_BIAS, false, false, 1>(d_X, d_Wt, d_bias, d_C, nullptr, M, N, K, N, st, nullptr, d_c1, (LnPartial*)d_stats);
    if (epi == 1) return launch_gemm_pp64<EPI_BIAS_GELU, false, false, 1>(d_X, d_Wt, d_bias, d_C, nullptr, M, N, K, N, st, nullptr, d_c1, (LnPartial*)d_stats);
    return VG_ERR_ARG;
}

int vg_gemm_trace(int var, const void* d_X, const void* d_Wt, const float* d_bias, void* d_C, int64_t* d_trace, int M, int N,
                  int K, int ldc, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    switch (var) {
        case 20: return launch_gemm_pp<EPI_BIAS, 4, true>(d_X, d_Wt, d_bias, d_C, nullptr, M, N, K, ldc, st, (long long*)d_trace);
        case 21: return launch_gemm_pp<EPI_BIAS, 5, true>(d_X, d_Wt, d_bias, d_C, nullptr, M, N, K, ldc, st, (long long*)d_trace);
        case 22: return launch_gemm_pp<EPI_BIAS, 4, true, 1>(d_X, d_Wt, d_bias, d_C, nullptr, M, N, K, ldc, st, (long long*)d_trace);
        case 23: return launch_gemm_pp<EPI_BIAS, 5, true, 1>(d_X, d_Wt, d_bias, d_C, nullptr, M, N, K, ldc, st, (long long*)d_trace);
        case 32: return launch_gemm_pp64<EPI_BIAS, true>(d_X, d_Wt, d_bias, d_C, nullptr, M, N, K, ldc, st, (long long*)d_trace);
        case 33: return launch_gemm_pp64<EPI_BIAS_GELU, true>(d_X, d_Wt, d_bias, d_C, nullptr, M, N, K, ldc, st, (long long*)d_trace);
        case 34: return launch_gemm_pp64<EPI_BIAS_RESID, true>(d_X, d_Wt, d_bias, nullptr, (float*)d_C, M, N, K, ldc, st, (long long*)d_trace);
        case 35: return launch_gemm_pp64<EPI_BIAS_RESID_H, true>(d_X, d_Wt, d_bias, nullptr, (float*)d_C, M, N, K, ldc, st, (long long*)d_trace);
        case 50: return launch_gemm_w4<EPI_BIAS, 0, VG_W4_TRACE_VAR>(d_X, d_Wt, d_bias, d_C, nullptr, M, N, K, ldc, st, nullptr, nullptr, nullptr, (long long*)d_trace);
        case 40: return launch_gemm_x2<EPI_BIAS, 0, true>(d_X, d_Wt, d_bias, d_C, nullptr, M, N, K, ldc, st, nullptr, nullptr, nullptr, (long long*)d_trace);
        default: return VG_ERR_ARG; }
    VG_LAUNCH_CHECK();
    return VG_OK;
}

/* development aid: k_attention_f16 alone (trace = null) or with per-wave phase cycle counts: d_trace receives, per (workgroup of the
 * persistent grid min(items, 256), wave 0..6), eight int64 (see the AT_STAMP comments in the kernel). */
int vg_attention_trace(const void* d_qkv, void* d_out, int n_crops, int T, int W, int heads, int ld, int64_t* d_trace, void* stream) {
    if (!d_qkv || !d_out || n_crops <= 0 || T > AT_MAXT || heads * 64 != W) return VG_ERR_ARG;
    const int items = n_crops * heads;
    hipStream_t st = (hipStream_t)stream;
    if (d_trace) return launch_attention<true>((const f16*)d_qkv, (f16*)d_out, T, W, heads, ld, items, (long long*)d_trace, st);
    return launch_attention<false>((const f16*)d_qkv, (f16*)d_out, T, W, heads, ld, items, nullptr, st);
}

}  // extern "C"
