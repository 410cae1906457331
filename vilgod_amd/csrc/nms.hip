// Rotated-box NMS for gfx950: the device counterpart of pcdet's iou3d_nms_utils.nms_gpu / nms_normal_gpu, the two functions of the
// module the reference imports (src/utils/tracking_utils.py:6, src/vilgod/zero_shot_detector.py:17, src/datasets/waymo_dataset.py:3)
// that had none here.  Grouped: one call runs an independent NMS over every group of rows [off[g], off[g + 1]).
//
//   k_nms_rank     one lane per row: its rank in its group under (score descending, row index ascending), by counting the keys that
//                  stand before it -- O(n^2) per group, deterministic, no sort network.  order[off[g] + rank] = row, or ~row (negative)
//                  for a row that can neither be kept nor suppress (NaN score, non-finite box value).
//   k_nms_mask     one workgroup per ranked row p, its four waves over the 64-column words w >= p / 64: lane l evaluates
//                  v(q = 64 w + l, p) for q > p and the word is the wave's ballot -- one vector store per word, no
//                  read-modify-write.  Only the upper triangle is computed; every word k_nms_reduce reads is written here.
//   k_nms_reduce   one wave per group.  Lane l holds word l of the `removed` set (VG_NMS_MAX_GROUP = 64 x 64 rows: one word per
//                  lane).  It walks the ranks in batches of NMS_BATCH: the next batch's mask rows and order entries are requested
//                  before the current batch is tested, so the serial chain is a readlane, a bit test and an OR per row, not a
//                  memory latency.  Lane 0 appends the kept rows; the tail is filled with -1 and the count written at the end.
//
// A group's geometry comes from the offset table ON THE DEVICE (nms_group): nothing is read back, nothing allocated, no atomics,
// and the grids depend on n_groups, n_rows and max_group alone, so a call can be captured into a graph.  A group the table does not
// describe properly (larger than max_group, reaching outside [0, n_rows), negative size) gets count -1 and -1 in those of its rows
// that exist.  The pair text is csrc/nms_pair.inc + csrc/iou_pair.inc; vg_boxes_nms_host runs it over host arrays, bit for bit.
#include <algorithm>
#include <vector>
#include "common.h"
#include "vilgod_hip.h"
#include "nms_pair.inc"

#define NMS_BLOCK 256
#define NMS_BATCH 16

struct NmsGroup {
    int o0, n, m;        // first row, rows, rows that take part (pre_max)
    int lo, hi;          // a bad group's rows inside [0, n_rows)
    bool bad;
};

VG_HD NmsGroup nms_group(const int32_t* __restrict__ off, int g, int n_rows, int max_group, int pre_max) {
    NmsGroup G;
    const int o0 = off[g], o1 = off[g + 1];
    G.bad = o0 < 0 || o1 < o0 || o1 > n_rows || o1 - o0 > max_group;
    G.o0 = o0;
    G.n = G.bad ? 0 : o1 - o0;
    G.m = pre_max > 0 && pre_max < G.n ? pre_max : G.n;
    G.lo = o0 < 0 ? 0 : (o0 > n_rows ? n_rows : o0);
    G.hi = o1 < 0 ? 0 : (o1 > n_rows ? n_rows : o1);
    return G;
}

template <typename T>
__host__ __device__ __forceinline__ void nms_load(const T* __restrict__ rows, int64_t i, double* v) {
    const T* r = rows + i * 7;
#pragma unroll
    for (int k = 0; k < 7; ++k) v[k] = (double)r[k];
}

template <typename TB, typename TS>
__global__ __launch_bounds__(NMS_BLOCK) void k_nms_rank(const TB* __restrict__ boxes, const TS* __restrict__ scores,
                                                        const int32_t* __restrict__ off, int n_rows, int max_group,
                                                        int32_t* __restrict__ order) {
    const NmsGroup G = nms_group(off, blockIdx.x, n_rows, max_group, 0);
    const int i = blockIdx.y * NMS_BLOCK + threadIdx.x;
    if (i >= G.n) return;
    const int row = G.o0 + i;
    const double si = (double)scores[row];
    int rank = 0;
    for (int j = 0; j < G.n; ++j) {
        const double sj = (double)scores[G.o0 + j];          // one address per wave
        rank += (j != i && nms_before(sj, j, si, i)) ? 1 : 0;
    }
    double v[7];
    nms_load(boxes, row, v);
    order[G.o0 + rank] = nms_row_ok(si, v) ? row : ~row;     // the ranks of a group are a permutation of 0 .. n - 1
}

template <typename TB>
__global__ __launch_bounds__(NMS_BLOCK) void k_nms_mask(const TB* __restrict__ boxes, const int32_t* __restrict__ off, int n_rows,
                                                        int max_group, int pre_max, int mode, double thresh,
                                                        const int32_t* __restrict__ order, unsigned long long* __restrict__ mask) {
    const NmsGroup G = nms_group(off, blockIdx.x, n_rows, max_group, pre_max);
    const int p = blockIdx.y;
    if (p >= G.m) return;
    const int W = (max_group + 63) >> 6, Wm = (G.m + 63) >> 6;
    const int wave = vg_uniform((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int op = order[G.o0 + p];
    double vb[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) vb[k] = 0.0;
    if (op >= 0) nms_load(boxes, op, vb);
    unsigned long long* __restrict__ mrow = mask + (int64_t)(G.o0 + p) * W;
    for (int w = (p >> 6) + wave; w < Wm; w += NMS_BLOCK / 64) {
        const int q = 64 * w + lane;
        bool hit = false;
        if (op >= 0 && q > p && q < G.m) {
            const int oq = order[G.o0 + q];
            if (oq >= 0) {
                double va[7];
                nms_load(boxes, oq, va);
                hit = nms_value(va, vb, mode) > thresh;      // strict; a NaN value compares false
            }
        }
        const unsigned long long word = __ballot(hit);
        if (lane == 0) mrow[w] = word;
    }
}

__device__ __forceinline__ unsigned long long nms_readlane64(unsigned long long v, int l) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, l);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l);
    return ((unsigned long long)hi << 32) | lo;
}

// rows base .. base + NMS_BATCH - 1 of the group: this lane's word of each mask row (0 where the row, or the word, is not one the
// mask kernel computed) and, in lane k, the order entry of row base + k (-1 behind the last row that takes part)
__device__ __forceinline__ void nms_fetch(const unsigned long long* __restrict__ mask, const int32_t* __restrict__ order, const NmsGroup& G,
                                          int W, int Wm, int lane, int base, unsigned long long* r, int& o) {
#pragma unroll
    for (int k = 0; k < NMS_BATCH; ++k) {
        const int p = base + k;
        r[k] = (p < G.m && lane >= (p >> 6) && lane < Wm) ? mask[(int64_t)(G.o0 + p) * W + lane] : 0ull;
    }
    o = (lane < NMS_BATCH && base + lane < G.m) ? order[G.o0 + base + lane] : -1;
}

__global__ __launch_bounds__(64) void k_nms_reduce(const int32_t* __restrict__ off, int n_rows, int max_group, int pre_max,
                                                   const int32_t* __restrict__ order, const unsigned long long* __restrict__ mask,
                                                   int32_t* __restrict__ keep, int32_t* __restrict__ count) {
    const int g = blockIdx.x, lane = threadIdx.x;
    const NmsGroup G = nms_group(off, g, n_rows, max_group, pre_max);
    if (G.bad) {
        for (int i = G.lo + lane; i < G.hi; i += 64) keep[i] = -1;
        if (lane == 0) count[g] = -1;
        return;
    }
    const int W = (max_group + 63) >> 6, Wm = (G.m + 63) >> 6;
    unsigned long long removed = 0ull, cur[NMS_BATCH], nxt[NMS_BATCH];
    int ocur, onxt, cnt = 0;
    nms_fetch(mask, order, G, W, Wm, lane, 0, cur, ocur);
    for (int base = 0; base < G.m; base += NMS_BATCH) {
        nms_fetch(mask, order, G, W, Wm, lane, base + NMS_BATCH, nxt, onxt);
#pragma unroll
        for (int k = 0; k < NMS_BATCH; ++k) {
            const int p = base + k;
            const int row = __builtin_amdgcn_readlane(ocur, k);              // wave-uniform
            if (row >= 0) {
                const unsigned long long word = nms_readlane64(removed, p >> 6);
                if (!((word >> (p & 63)) & 1ull)) {
                    if (lane == 0) keep[G.o0 + cnt] = row;
                    ++cnt;
                    removed |= cur[k];
                }
            }
        }
#pragma unroll
        for (int k = 0; k < NMS_BATCH; ++k) cur[k] = nxt[k];
        ocur = onxt;
    }
    for (int i = cnt + lane; i < G.n; i += 64) keep[G.o0 + i] = -1;
    if (lane == 0) count[g] = cnt;
}

static inline size_t nms_order_bytes(int n_rows) { return ((size_t)n_rows * sizeof(int32_t) + 7) & ~(size_t)7; }

extern "C" size_t vg_boxes_nms_work_bytes(int n_rows, int max_group, int n_groups) {
    if (n_rows <= 0 || max_group <= 0 || n_groups <= 0) return 0;
    return nms_order_bytes(n_rows) + (size_t)n_rows * (size_t)((max_group + 63) >> 6) * sizeof(unsigned long long);
}

static int nms_check(int box_dtype, int score_dtype, int n_groups, int n_rows, int max_group, int mode) {
    if (box_dtype != VG_NMS_F32 && box_dtype != VG_NMS_F64) return VG_ERR_ARG;
    if (score_dtype != VG_NMS_F32 && score_dtype != VG_NMS_F64) return VG_ERR_ARG;
    if (mode != VG_NMS_ROTATED && mode != VG_NMS_NORMAL) return VG_ERR_ARG;
    if (n_groups < 0 || n_rows < 0 || max_group < 0 || max_group > VG_NMS_MAX_GROUP) return VG_ERR_ARG;
    return VG_OK;
}

template <typename TB, typename TS>
static void nms_launch(const void* d_boxes, const void* d_scores, const int32_t* d_off, int n_groups, int n_rows, int max_group, int mode,
                       double thresh, int pre_max, void* d_work, int32_t* d_keep, int32_t* d_count, hipStream_t st) {
    int32_t* order = (int32_t*)d_work;
    unsigned long long* mask = (unsigned long long*)((char*)d_work + nms_order_bytes(n_rows));
    if (max_group > 0) {
        hipLaunchKernelGGL((k_nms_rank<TB, TS>), dim3((unsigned)n_groups, (unsigned)vg_div_up(max_group, NMS_BLOCK)), dim3(NMS_BLOCK), 0, st,
                           (const TB*)d_boxes, (const TS*)d_scores, d_off, n_rows, max_group, order);
        const int rows = pre_max > 0 && pre_max < max_group ? pre_max : max_group;       // ranks that can take part
        hipLaunchKernelGGL(k_nms_mask<TB>, dim3((unsigned)n_groups, (unsigned)rows), dim3(NMS_BLOCK), 0, st, (const TB*)d_boxes, d_off, n_rows,
                           max_group, pre_max, mode, thresh, order, mask);
    }
    hipLaunchKernelGGL(k_nms_reduce, dim3((unsigned)n_groups), dim3(64), 0, st, d_off, n_rows, max_group, pre_max, order, mask, d_keep,
                       d_count);
}

extern "C" int vg_boxes_nms(int box_dtype, const void* d_boxes, int score_dtype, const void* d_scores, const int32_t* d_off, int n_groups,
                            int n_rows, int max_group, int mode, double thresh, int pre_max, void* d_work, int32_t* d_keep,
                            int32_t* d_count, void* stream) {
    if (nms_check(box_dtype, score_dtype, n_groups, n_rows, max_group, mode) != VG_OK) return VG_ERR_ARG;
    if (n_groups == 0 || n_rows == 0) return VG_OK;
    if (!d_boxes || !d_scores || !d_off || !d_keep || !d_count || (max_group > 0 && !d_work)) return VG_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (box_dtype == VG_NMS_F32 && score_dtype == VG_NMS_F32)
        nms_launch<float, float>(d_boxes, d_scores, d_off, n_groups, n_rows, max_group, mode, thresh, pre_max, d_work, d_keep, d_count, st);
    else if (box_dtype == VG_NMS_F32)
        nms_launch<float, double>(d_boxes, d_scores, d_off, n_groups, n_rows, max_group, mode, thresh, pre_max, d_work, d_keep, d_count, st);
    else if (score_dtype == VG_NMS_F32)
        nms_launch<double, float>(d_boxes, d_scores, d_off, n_groups, n_rows, max_group, mode, thresh, pre_max, d_work, d_keep, d_count, st);
    else
        nms_launch<double, double>(d_boxes, d_scores, d_off, n_groups, n_rows, max_group, mode, thresh, pre_max, d_work, d_keep, d_count, st);
    VG_LAUNCH_CHECK();
    return VG_OK;
}

// the same rules, one group after the other: the ranking by std::sort under nms_before, the greedy pass evaluating v(q, p) against
// the kept rows only (the value of a pair does not depend on which other pairs are evaluated)
template <typename TB, typename TS>
static void nms_host_groups(const TB* boxes, const TS* scores, const int32_t* off, int n_groups, int n_rows, int max_group, int mode,
                            double thresh, int pre_max, int32_t* keep, int32_t* count) {
    std::vector<int> order, kept;
    for (int g = 0; g < n_groups; ++g) {
        const NmsGroup G = nms_group(off, g, n_rows, max_group, pre_max);
        if (G.bad) {
            for (int i = G.lo; i < G.hi; ++i) keep[i] = -1;
            count[g] = -1;
            continue;
        }
        order.resize(G.n);
        for (int i = 0; i < G.n; ++i) order[i] = i;
        const TS* s = scores + G.o0;
        std::sort(order.begin(), order.end(), [s](int j, int i) { return j != i && nms_before((double)s[j], j, (double)s[i], i); });
        kept.clear();
        for (int r = 0; r < G.m; ++r) {
            const int row = G.o0 + order[r];
            double va[7], vb[7];
            nms_load(boxes, row, va);
            if (!nms_row_ok((double)scores[row], va)) continue;
            bool gone = false;
            for (size_t k = 0; k < kept.size() && !gone; ++k) {
                nms_load(boxes, kept[k], vb);
                gone = nms_value(va, vb, mode) > thresh;
            }
            if (!gone) kept.push_back(row);
        }
        for (int i = 0; i < G.n; ++i) keep[G.o0 + i] = i < (int)kept.size() ? kept[i] : -1;
        count[g] = (int32_t)kept.size();
    }
}

extern "C" int vg_boxes_nms_host(int box_dtype, const void* h_boxes, int score_dtype, const void* h_scores, const int32_t* h_off,
                                 int n_groups, int n_rows, int max_group, int mode, double thresh, int pre_max, int32_t* h_keep,
                                 int32_t* h_count) {
    if (nms_check(box_dtype, score_dtype, n_groups, n_rows, max_group, mode) != VG_OK) return VG_ERR_ARG;
    if (n_groups == 0 || n_rows == 0) return VG_OK;
    if (!h_boxes || !h_scores || !h_off || !h_keep || !h_count) return VG_ERR_ARG;
    if (box_dtype == VG_NMS_F32 && score_dtype == VG_NMS_F32)
        nms_host_groups((const float*)h_boxes, (const float*)h_scores, h_off, n_groups, n_rows, max_group, mode, thresh, pre_max, h_keep, h_count);
    else if (box_dtype == VG_NMS_F32)
        nms_host_groups((const float*)h_boxes, (const double*)h_scores, h_off, n_groups, n_rows, max_group, mode, thresh, pre_max, h_keep, h_count);
    else if (score_dtype == VG_NMS_F32)
        nms_host_groups((const double*)h_boxes, (const float*)h_scores, h_off, n_groups, n_rows, max_group, mode, thresh, pre_max, h_keep, h_count);
    else
        nms_host_groups((const double*)h_boxes, (const double*)h_scores, h_off, n_groups, n_rows, max_group, mode, thresh, pre_max, h_keep, h_count);
    return VG_OK;
}
