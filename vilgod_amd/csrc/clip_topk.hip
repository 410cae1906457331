// Top-k classes per crop for gfx950: what clip_utils.py:49-61 does on the host with np.argpartition + np.argsort over the
// probability table, on the device next to the kernels that wrote the table (vg_clip_scores / vg_clip_scores_wide).
//
//   k_clip_topk   one wave per crop.  Lane l owns classes l, l + 64, ... and holds in registers its best entry that has not been
//                 taken yet (`cur`).  Each of the top_k rounds is one 6-step shuffle butterfly over the (probability, class) key --
//                 the argmax at the end of k_clip_scores under clip_topk_before -- after which every lane knows the winner; lane 0
//                 stores it.  Only the lane that owned the winner needs a new `cur`: the best entry of ITS classes strictly behind
//                 the key just taken (the order is strict and total, so "behind the last one taken" is "not taken yet": no flags).
//                 The wave looks for it together, lane j reading class (winner % 64) + 64 j (+ 4096 per further pass), and a second
//                 butterfly hands the result to the owner: one load per lane up to 4096 classes instead of 64 by one lane.
//                 All branches are wave-uniform; the row is read once by the whole wave and once per round in one stride.
//
// One launch on the caller's stream, grid = n: no atomics, no read-back, no allocation, no scratch, no LDS; the same bits on every
// run; capturable.  Compiler's kernel metadata (gfx950, -O3): 23 VGPRs, 29 SGPRs, 0 bytes of LDS, 0 bytes of scratch.
// vg_clip_topk_host orders the same rows with std::partial_sort under the same comparator: identical indices and score bits.
#include <algorithm>
#include <vector>
#include "common.h"
#include "vilgod_hip.h"
#include "clip_topk_key.inc"

// the wave's first entry under clip_topk_before, in every lane
__device__ __forceinline__ void clip_topk_wave_first(float& p, int& i) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float op = __shfl_xor(p, o);
        const int oi = __shfl_xor(i, o);
        if (clip_topk_before(op, oi, p, i)) {
            p = op;
            i = oi;
        }
    }
}

__global__ __launch_bounds__(64) void k_clip_topk(const float* __restrict__ probs, int Kc, int top_k, int32_t* __restrict__ idx,
                                                  float* __restrict__ score) {
    const int lane = threadIdx.x;
    const float* __restrict__ row = probs + (size_t)blockIdx.x * Kc;
    int32_t* __restrict__ oi = idx + (size_t)blockIdx.x * top_k;
    float* __restrict__ os = score + (size_t)blockIdx.x * top_k;
    const float none = __int_as_float(0x7fc00000);
    float cp = none;
    int ci = CLIP_TOPK_NONE;
    for (unsigned c = lane; c < (unsigned)Kc; c += 64) {          // (unsigned: c + 64 cannot wrap for any int Kc)
        const float p = row[c];
        if (clip_topk_before(p, (int)c, cp, ci)) {
            cp = p;
            ci = (int)c;
        }
    }
    for (int r = 0; r < top_k; ++r) {
        float bp = cp;
        int bi = ci;
        clip_topk_wave_first(bp, bi);                 // top_k <= Kc: a real class
        if (lane == 0) {
            oi[r] = bi;
            os[r] = bp;
        }
        if (r + 1 == top_k) break;
        const int owner = bi & 63;
        float np_ = none;
        int ni = CLIP_TOPK_NONE;
        for (unsigned c = owner + 64 * lane; c < (unsigned)Kc; c += 64 * 64) {
            const float p = row[c];
            if (clip_topk_before(bp, bi, p, (int)c) && clip_topk_before(p, (int)c, np_, ni)) {
                np_ = p;
                ni = (int)c;
            }
        }
        clip_topk_wave_first(np_, ni);
        if (lane == owner) {
            cp = np_;
            ci = ni;
        }
    }
}

static int clip_topk_check(const float* probs, int n, int n_classes, int top_k, const int32_t* idx, const float* score) {
    if (top_k < 1 || top_k > VG_CLIP_MAX_TOPK || n_classes < 1 || top_k > n_classes) return VG_ERR_ARG;
    if (n > 0 && (!probs || !idx || !score)) return VG_ERR_ARG;
    return VG_OK;
}

extern "C" int vg_clip_topk(const float* d_probs, int n, int n_classes, int top_k, int32_t* d_idx, float* d_score, void* stream) {
    if (clip_topk_check(d_probs, n, n_classes, top_k, d_idx, d_score) != VG_OK) return VG_ERR_ARG;
    if (n <= 0) return VG_OK;
    hipLaunchKernelGGL(k_clip_topk, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream, d_probs, n_classes, top_k, d_idx, d_score);
    VG_LAUNCH_CHECK();
    return VG_OK;
}

extern "C" int vg_clip_topk_host(const float* h_probs, int n, int n_classes, int top_k, int32_t* h_idx, float* h_score) {
    if (clip_topk_check(h_probs, n, n_classes, top_k, h_idx, h_score) != VG_OK) return VG_ERR_ARG;
    std::vector<int32_t> order((size_t)n_classes);
    for (int i = 0; i < n; ++i) {
        const float* row = h_probs + (size_t)i * n_classes;
        for (int c = 0; c < n_classes; ++c) order[c] = c;
        std::partial_sort(order.begin(), order.begin() + top_k, order.end(),
                          [row](int32_t a, int32_t b) { return a != b && clip_topk_before(row[a], a, row[b], b); });
        for (int r = 0; r < top_k; ++r) {
            h_idx[(size_t)i * top_k + r] = order[r];
            h_score[(size_t)i * top_k + r] = row[order[r]];
        }
    }
    return VG_OK;
}
