// Development build only (-DVG_DEV, libvilgod_hip_dev.so): included by ../vit_gemm_launch.inc in place.
// Tile-order sweeps and the half-grid experiment, read per launch: gemm_tile_chunk hands over the product's choice of column tiles per
// L2 chunk (and, for the persistent k_gemm_f16_w4, the grid's workgroups) and launches with what is left in them.
static void dev_tile_order(int fam, int N, int* cwt, int* cap) {
    if (fam == GF_F16) {
        if (getenv("VG_GEMM_NO_CHUNK")) *cwt = N / GBN;
        return;
    }
    const int ntn = N / 256;
    if (fam == GF_PP64) {
        if (getenv("VG_GEMM_CW")) { *cwt = env_int("VG_GEMM_CW", 0); if (*cwt < 1 || ntn % *cwt) *cwt = ntn; }
        return;
    }
    if (cap) { const int half = env_int("VG_GEMM_W4_GRID", 0); if (half >= 8 && half < *cap) *cap = half; }   // experiment: two encodes on disjoint CU halves
    { const int c = env_int("VG_GEMM_CW", 0); if (c >= 1 && ntn % c == 0) *cwt = c; }
}
