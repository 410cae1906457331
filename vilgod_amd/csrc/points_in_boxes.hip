// Points-in-boxes for gfx950: the device counterpart of pcdet's roiaware_pool3d_utils.points_in_boxes_gpu, which the reference reaches
// in src/utils/pointcloud_utils.py:144-158 (get_box_heights) and :516-522 (points_in_boxes; src/vilgod/lidar_frame.py:160 turns box
// proposals into detections with it).  Per point: the LOWEST index of a box that contains it, -1 when none does.
//
//   k_points_in_boxes   one lane per point, 256-thread workgroups, blockIdx.y = batch element.  The boxes go through LDS in chunks of
//                       PIB_CHUNK (256 boxes x 9 doubles = 18 KB, structure of arrays): thread t of the workgroup prepares box t of
//                       the chunk (csrc/points_in_boxes_pair.inc pib_prepare: halves with the margin, sine / cosine, squared reject
//                       radius), then every lane walks the chunk in ascending order with broadcast LDS reads (all lanes read the same
//                       word: no bank conflict) -- radius reject, z test, rotation -- and stops testing at its first hit.  The chunk
//                       loop's trip count depends on n_boxes alone, so every thread meets every barrier: a lane that has its box, or
//                       one beyond n_points, still prepares its box of the next chunk.  The last chunk is walked up to the number of
//                       boxes it holds: there are no padding boxes and no infinite constants.
//
// No atomics, no read-back, no allocation: one launch on the caller's stream (capturable), the same bits on every run.
// vg_points_in_boxes_host runs the same pair body over host arrays; the two agree bit for bit (no library maths, no contraction).
#include <vector>
#include "common.h"
#include "vilgod_hip.h"
#include "points_in_boxes_pair.inc"

#define PIB_BLOCK 256
#define PIB_CHUNK VG_PIB_CHUNK
static_assert(PIB_CHUNK == PIB_BLOCK, "thread t prepares box t of the chunk");

template <typename T>
__host__ __device__ __forceinline__ void pib_load(const T* __restrict__ rows, int64_t i, double* v) {
    const T* r = rows + i * 7;
#pragma unroll
    for (int k = 0; k < 7; ++k) v[k] = (double)r[k];
}

// box j of the chunk in LDS, read word by word as pib_inside asks for them
struct PibLdsView {
    const double (*sh)[PIB_CHUNK];
    int j;
    __device__ __forceinline__ double cx() const { return sh[0][j]; }
    __device__ __forceinline__ double cy() const { return sh[1][j]; }
    __device__ __forceinline__ double cz() const { return sh[2][j]; }
    __device__ __forceinline__ double hx() const { return sh[3][j]; }
    __device__ __forceinline__ double hy() const { return sh[4][j]; }
    __device__ __forceinline__ double hz() const { return sh[5][j]; }
    __device__ __forceinline__ double cs() const { return sh[6][j]; }
    __device__ __forceinline__ double sn() const { return sh[7][j]; }
    __device__ __forceinline__ double r2() const { return sh[8][j]; }
};

template <typename T>
__global__ __launch_bounds__(PIB_BLOCK) void k_points_in_boxes(const float* __restrict__ points, int point_stride, int n_points,
                                                               const T* __restrict__ boxes, int n_boxes,
                                                               int32_t* __restrict__ box_idx) {
    __shared__ double sh[9][PIB_CHUNK];
    const int t = threadIdx.x;
    const int i = blockIdx.x * PIB_BLOCK + t;                        // n_points <= 2^31 - 1 and the grid covers it once: no overflow
    const int64_t b = blockIdx.y;
    const bool live = i < n_points;
    double x = 0.0, y = 0.0, z = 0.0;
    if (live) {
        const float* p = points + (b * n_points + i) * (int64_t)point_stride;
        x = (double)p[0]; y = (double)p[1]; z = (double)p[2];
    }
    int found = live ? -1 : 0;                                        // a lane without a point tests nothing
    const T* bx = boxes + b * n_boxes * 7;
    for (int base = 0; base < n_boxes; base += PIB_CHUNK) {           // uniform over the workgroup
        const int nb = min(PIB_CHUNK, n_boxes - base);
        if (t < nb) {
            double v[7];
            PibBox o;
            pib_load(bx, (int64_t)base + t, v);
            pib_prepare(v, o);
            sh[0][t] = o.cx; sh[1][t] = o.cy; sh[2][t] = o.cz;
            sh[3][t] = o.hx; sh[4][t] = o.hy; sh[5][t] = o.hz;
            sh[6][t] = o.cs; sh[7][t] = o.sn; sh[8][t] = o.r2;
        }
        __syncthreads();
        for (int j = 0; j < nb && found < 0; ++j)
            if (pib_inside(PibLdsView{sh, j}, x, y, z)) found = base + j;
        __syncthreads();                                              // the next chunk overwrites sh
    }
    if (live) box_idx[b * n_points + i] = found;
}

static int pib_check(int box_dtype, const void* points, int point_stride, int n_points, const void* boxes, int n_boxes, int batch,
                     const void* box_idx, bool& nothing) {
    nothing = true;
    if (box_dtype != VG_PIB_F32 && box_dtype != VG_PIB_F64) return VG_ERR_ARG;
    if (n_points < 0 || n_boxes < 0 || batch < 0 || point_stride < 3) return VG_ERR_ARG;
    if (n_points == 0 || batch == 0) return VG_OK;
    if (!points || !box_idx || (n_boxes > 0 && !boxes)) return VG_ERR_ARG;
    nothing = false;
    return VG_OK;
}

extern "C" int vg_points_in_boxes(int box_dtype, const float* d_points, int point_stride, int n_points, const void* d_boxes, int n_boxes,
                                  int batch, int32_t* d_box_idx, void* stream) {
    bool nothing;
    const int rc = pib_check(box_dtype, d_points, point_stride, n_points, d_boxes, n_boxes, batch, d_box_idx, nothing);
    if (rc != VG_OK || nothing) return rc;
    if (batch > 65535) return VG_ERR_CAPACITY;                        // grid.y
    const dim3 grid((unsigned)(((int64_t)n_points + PIB_BLOCK - 1) / PIB_BLOCK), (unsigned)batch);
    hipStream_t st = (hipStream_t)stream;
    if (box_dtype == VG_PIB_F32)
        hipLaunchKernelGGL(k_points_in_boxes<float>, grid, dim3(PIB_BLOCK), 0, st, d_points, point_stride, n_points,
                           (const float*)d_boxes, n_boxes, d_box_idx);
    else
        hipLaunchKernelGGL(k_points_in_boxes<double>, grid, dim3(PIB_BLOCK), 0, st, d_points, point_stride, n_points,
                           (const double*)d_boxes, n_boxes, d_box_idx);
    VG_LAUNCH_CHECK();
    return VG_OK;
}

template <typename T>
static void pib_host(const float* points, int point_stride, int n_points, const T* boxes, int n_boxes, int batch, int32_t* box_idx) {
    std::vector<PibBox> prep((size_t)n_boxes);
    for (int64_t b = 0; b < batch; ++b) {
        for (int j = 0; j < n_boxes; ++j) {
            double v[7];
            pib_load(boxes, b * n_boxes + j, v);
            pib_prepare(v, prep[j]);
        }
        for (int64_t i = 0; i < n_points; ++i) {
            const float* p = points + (b * n_points + i) * (int64_t)point_stride;
            const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
            int found = -1;
            for (int j = 0; j < n_boxes && found < 0; ++j)
                if (pib_inside(PibBoxView{prep[j]}, x, y, z)) found = j;
            box_idx[b * n_points + i] = found;
        }
    }
}

extern "C" int vg_points_in_boxes_host(int box_dtype, const float* h_points, int point_stride, int n_points, const void* h_boxes,
                                       int n_boxes, int batch, int32_t* h_box_idx) {
    bool nothing;
    const int rc = pib_check(box_dtype, h_points, point_stride, n_points, h_boxes, n_boxes, batch, h_box_idx, nothing);
    if (rc != VG_OK || nothing) return rc;
    if (box_dtype == VG_PIB_F32)
        pib_host(h_points, point_stride, n_points, (const float*)h_boxes, n_boxes, batch, h_box_idx);
    else
        pib_host(h_points, point_stride, n_points, (const double*)h_boxes, n_boxes, batch, h_box_idx);
    return VG_OK;
}
