// Rotated-box IoU for gfx950: the device counterpart of pcdet's boxes_iou3d_gpu / boxes_iou_bev, which the reference calls in
// src/utils/tracking_utils.py:9-20, src/vilgod/zero_shot_detector.py:737-739 and src/datasets/waymo_dataset.py:300.
//
//   k_boxes_iou   one lane per pair, many independent [na_g, nb_g] matrices per launch.  The lanes are laid over the OUTPUT range
//                 [out_off[0], end of the last group): lane t owns output element out_off[0] + t, finds its group by a binary
//                 search in out_off (non-decreasing, ranges disjoint: checked on the host before the launch) and leaves an element
//                 that belongs to no group -- slack between two groups -- untouched.  A thousand 1 x 1 groups are four
//                 workgroups, not a thousand.
//
// The pair body is csrc/iou_pair.inc (all float64, float32 rows widened exactly); vg_boxes_iou3d_host runs the same body over host
// arrays, and the two agree bit for bit (no library maths, no contraction).  Registers only: no LDS, no scratch.
#include <vector>
#include "common.h"
#include "vilgod_hip.h"
#include "iou_pair.inc"

#define IOU_BLOCK 256

template <typename T>
__host__ __device__ __forceinline__ void iou_load(const T* __restrict__ rows, int64_t i, double* v) {
    const T* r = rows + i * 7;
#pragma unroll
    for (int k = 0; k < 7; ++k) v[k] = (double)r[k];
}

template <typename T>
__global__ __launch_bounds__(IOU_BLOCK) void k_boxes_iou(const T* __restrict__ a, const int32_t* __restrict__ a_off,
                                                         const T* __restrict__ b, const int32_t* __restrict__ b_off, int n_groups,
                                                         const int64_t* __restrict__ out_off, int64_t first, int64_t span, int mode,
                                                         double* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * IOU_BLOCK + threadIdx.x;
    if (t >= span) return;
    const int64_t p = first + t;
    int lo = 0, hi = n_groups - 1;                   // the last group that starts at or before p (out_off[0] == first <= p)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (out_off[mid] <= p) lo = mid; else hi = mid - 1;
    }
    const int a0 = a_off[lo], b0 = b_off[lo];
    const int64_t na = a_off[lo + 1] - a0, nb = b_off[lo + 1] - b0;
    const int64_t local = p - out_off[lo];
    if (nb <= 0 || local >= na * nb) return;         // slack behind the group (or an empty group)
    const int64_t i = local / nb, j = local - i * nb;
    double va[7], vb[7];
    iou_load(a, a0 + i, va);
    iou_load(b, b0 + j, vb);
    out[p] = iou_pair(va, vb, mode);
}

// the offsets of both forms: a_off / b_off non-decreasing from >= 0, out_off >= 0 and every group's range behind the one before.
// -> VG_OK and the output span [first, end) of the non-empty work (first == end: nothing to do)
static int iou_check(const int32_t* a_off, const int32_t* b_off, const int64_t* out_off, int n_groups, int64_t& first, int64_t& end) {
    first = end = 0;
    if (a_off[0] < 0 || b_off[0] < 0) return VG_ERR_ARG;
    int64_t prev_end = 0;
    for (int g = 0; g < n_groups; ++g) {
        const int64_t na = (int64_t)a_off[g + 1] - a_off[g], nb = (int64_t)b_off[g + 1] - b_off[g];
        if (na < 0 || nb < 0 || out_off[g] < prev_end) return VG_ERR_ARG;
        prev_end = out_off[g] + na * nb;
    }
    first = out_off[0];
    end = prev_end;
    bool any = false;
    for (int g = 0; g < n_groups && !any; ++g) any = a_off[g + 1] > a_off[g] && b_off[g + 1] > b_off[g];
    if (!any) end = first;
    return VG_OK;
}

extern "C" int vg_boxes_iou3d(int dtype, const void* d_a, const int32_t* d_a_off, const void* d_b, const int32_t* d_b_off, int n_groups,
                              const int64_t* d_out_off, int mode, double* d_out, void* stream) {
    if (dtype != VG_IOU_F32 && dtype != VG_IOU_F64) return VG_ERR_ARG;
    if (mode != VG_IOU_3D && mode != VG_IOU_BEV && mode != VG_IOU_BEV_AREA) return VG_ERR_ARG;
    if (n_groups < 0) return VG_ERR_ARG;
    if (n_groups == 0) return VG_OK;
    if (!d_a_off || !d_b_off || !d_out_off) return VG_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    // the group table is small and decides the grid: read it back (this entry point synchronises the stream once)
    std::vector<int32_t> a_off(n_groups + 1), b_off(n_groups + 1);
    std::vector<int64_t> out_off(n_groups);
    VG_CHECK(hipMemcpyAsync(a_off.data(), d_a_off, sizeof(int32_t) * (n_groups + 1), hipMemcpyDeviceToHost, st));
    VG_CHECK(hipMemcpyAsync(b_off.data(), d_b_off, sizeof(int32_t) * (n_groups + 1), hipMemcpyDeviceToHost, st));
    VG_CHECK(hipMemcpyAsync(out_off.data(), d_out_off, sizeof(int64_t) * n_groups, hipMemcpyDeviceToHost, st));
    VG_CHECK(hipStreamSynchronize(st));
    int64_t first, end;
    if (iou_check(a_off.data(), b_off.data(), out_off.data(), n_groups, first, end) != VG_OK) return VG_ERR_ARG;
    if (end == first) return VG_OK;
    if (!d_a || !d_b || !d_out) return VG_ERR_ARG;
    const int64_t span = end - first, blocks = (span + IOU_BLOCK - 1) / IOU_BLOCK;
    if (blocks > 0x7fffffffLL) return VG_ERR_CAPACITY;
    if (dtype == VG_IOU_F32)
        hipLaunchKernelGGL(k_boxes_iou<float>, dim3((unsigned)blocks), dim3(IOU_BLOCK), 0, st, (const float*)d_a, d_a_off, (const float*)d_b,
                           d_b_off, n_groups, d_out_off, first, span, mode, d_out);
    else
        hipLaunchKernelGGL(k_boxes_iou<double>, dim3((unsigned)blocks), dim3(IOU_BLOCK), 0, st, (const double*)d_a, d_a_off,
                           (const double*)d_b, d_b_off, n_groups, d_out_off, first, span, mode, d_out);
    VG_LAUNCH_CHECK();
    return VG_OK;
}

template <typename T>
static void iou_host_groups(const T* a, const int32_t* a_off, const T* b, const int32_t* b_off, int n_groups, const int64_t* out_off,
                            int mode, double* out) {
    for (int g = 0; g < n_groups; ++g) {
        const int64_t na = a_off[g + 1] - a_off[g], nb = b_off[g + 1] - b_off[g];
        for (int64_t i = 0; i < na; ++i) {
            double va[7], vb[7];
            iou_load(a, a_off[g] + i, va);
            for (int64_t j = 0; j < nb; ++j) {
                iou_load(b, b_off[g] + j, vb);
                out[out_off[g] + i * nb + j] = iou_pair(va, vb, mode);
            }
        }
    }
}

extern "C" int vg_boxes_iou3d_host(int dtype, const void* h_a, const int32_t* h_a_off, const void* h_b, const int32_t* h_b_off,
                                   int n_groups, const int64_t* h_out_off, int mode, double* h_out) {
    if (dtype != VG_IOU_F32 && dtype != VG_IOU_F64) return VG_ERR_ARG;
    if (mode != VG_IOU_3D && mode != VG_IOU_BEV && mode != VG_IOU_BEV_AREA) return VG_ERR_ARG;
    if (n_groups < 0) return VG_ERR_ARG;
    if (n_groups == 0) return VG_OK;
    if (!h_a_off || !h_b_off || !h_out_off) return VG_ERR_ARG;
    int64_t first, end;
    if (iou_check(h_a_off, h_b_off, h_out_off, n_groups, first, end) != VG_OK) return VG_ERR_ARG;
    if (end == first) return VG_OK;
    if (!h_a || !h_b || !h_out) return VG_ERR_ARG;
    if (dtype == VG_IOU_F32)
        iou_host_groups((const float*)h_a, h_a_off, (const float*)h_b, h_b_off, n_groups, h_out_off, mode, h_out);
    else
        iou_host_groups((const double*)h_a, h_a_off, (const double*)h_b, h_b_off, n_groups, h_out_off, mode, h_out);
    return VG_OK;
}
