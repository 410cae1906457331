// Oriented extents of tracked clusters for gfx950: the per-point part of the motion-aligned boxes of moving tracks, the `else` branch
// of the reference's fit_bounding_boxes_simple (src/vilgod/zero_shot_detector.py:576-603): every cluster of a moving track is shifted
// by its float32 median, turned into the track's direction of travel, and measured -- min / max of x', y' and of the points' own z.
// The arithmetic per point is csrc/oriented_extent_point.inc (np.dot's float32 subtraction and float64 fused chain, restated); the
// O(entries) rest of the box (corners, sizes, top-3 median, closest-corner shift) stays host code in vilgod_amd/tracking.py.
//
//   k_cluster_oriented_extents   one workgroup of VG_OEXT_BLOCK threads (16 waves) per PAIR (cluster, rotation); the same cluster may
//                                sit in several pairs.  Every thread starts from the cluster's first point (one broadcast load) and
//                                folds in the points lo + t, lo + t + B, ...: four index loads, then four row gathers per trip, the
//                                positions clamped to the segment's last element -- a point folded in twice changes no minimum or
//                                maximum, so the loop has no tail and reads nothing outside [lo, hi).  Then a wave butterfly
//                                (__shfl_xor), one LDS step across the 16 waves, and threads 0..5 write the six values.
//
// A cluster is never split over workgroups, so there is no second pass and no atomic.  Minimum and maximum of finite values with one
// sign of zero (the point body folds zeros in as +0) do not depend on the order of combination: the same bits on every run, for every
// launch shape, and the same bits as the sequential host loop.  No ordered sum exists anywhere.
// One launch on the caller's stream, no read-back, no allocation, no synchronisation: it can be captured into a graph.
#include "common.h"
#include "vilgod_hip.h"
#include "oriented_extent_point.inc"

#define OEXT_BLOCK VG_OEXT_BLOCK
#define OEXT_WAVES (OEXT_BLOCK / WAVE)
#define OEXT_UNROLL 4
static_assert(OEXT_BLOCK % WAVE == 0 && OEXT_BLOCK <= 1024 && OEXT_WAVES >= 1, "whole waves, one workgroup");

__global__ __launch_bounds__(OEXT_BLOCK) void k_cluster_oriented_extents(const float* __restrict__ pts, int stride,
                                                                         const int32_t* __restrict__ idx, const int32_t* __restrict__ seg,
                                                                         int n_clusters, const int32_t* __restrict__ pair_cluster,
                                                                         const float* __restrict__ center3, const double* __restrict__ rot4,
                                                                         double* __restrict__ ext6) {
    __shared__ double sh[6][OEXT_WAVES];
    __shared__ int shbad[OEXT_WAVES];
    const int t = threadIdx.x;
    const int64_t p = blockIdx.x;
    const int c = pair_cluster ? pair_cluster[p] : (int)p;
    double* out = ext6 + p * 6;
    int64_t lo = 0, hi = 0;
    if (c >= 0 && c < n_clusters) {                                    // a pair index out of range reads no segment and no point
        lo = seg[c];
        hi = seg[c + 1];
    }
    const float cx = center3[p * 3 + 0], cy = center3[p * 3 + 1], cz = center3[p * 3 + 2];
    if (hi <= lo || !(oext_finite(cx) && oext_finite(cy) && oext_finite(cz))) {      // uniform over the workgroup: nobody waits at a barrier
        if (t < 6) out[t] = __builtin_nan("");
        return;
    }
    const OextRot rot = {rot4[p * 4 + 0], rot4[p * 4 + 1], rot4[p * 4 + 2], rot4[p * 4 + 3]};
    const int64_t last = hi - 1;
    OextAcc a;
    double q[3];
    {
        const float* r = pts + (int64_t)idx[lo] * stride;
        oext_first(a, q, oext_point(r[0], r[1], r[2], cx, cy, rot, q));
    }
    for (int64_t base = lo + t; base < hi; base += (int64_t)OEXT_UNROLL * OEXT_BLOCK) {
        int32_t id[OEXT_UNROLL];
        float x[OEXT_UNROLL], y[OEXT_UNROLL], z[OEXT_UNROLL];
#pragma unroll
        for (int u = 0; u < OEXT_UNROLL; ++u) {
            const int64_t i = base + (int64_t)u * OEXT_BLOCK;
            id[u] = idx[i < last ? i : last];
        }
#pragma unroll
        for (int u = 0; u < OEXT_UNROLL; ++u) {
            const float* r = pts + (int64_t)id[u] * stride;
            x[u] = r[0]; y[u] = r[1]; z[u] = r[2];
        }
#pragma unroll
        for (int u = 0; u < OEXT_UNROLL; ++u) oext_fold(a, q, oext_point(x[u], y[u], z[u], cx, cy, rot, q));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        OextAcc b;
#pragma unroll
        for (int k = 0; k < 6; ++k) b.v[k] = __shfl_xor(a.v[k], o);
        b.bad = __shfl_xor(a.bad, o);
        oext_merge(a, b);
    }
    if ((t & (WAVE - 1)) == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) sh[k][t / WAVE] = a.v[k];
        shbad[t / WAVE] = a.bad;
    }
    __syncthreads();
    if (t < 6) {
        double v = sh[t][0];
        int bad = shbad[0];
        for (int w = 1; w < OEXT_WAVES; ++w) {
            v = (t & 1) ? oext_max(v, sh[t][w]) : oext_min(v, sh[t][w]);
            bad |= shbad[w];
        }
        out[t] = bad ? __builtin_nan("") : v;
    }
}

static int oext_check(const void* points, int stride, const void* index, const void* seg_off, int n_clusters, const void* pair_cluster,
                      int n_pairs, const void* center3, const void* rot4, const void* ext6, bool& nothing) {
    nothing = true;
    if (n_clusters < 0 || n_pairs < 0 || stride < 3) return VG_ERR_ARG;
    if (n_pairs == 0) return VG_OK;                                     // (an empty pair list has no address: no identity is meant)
    if (!pair_cluster && n_pairs != n_clusters) return VG_ERR_ARG;
    if (!center3 || !rot4 || !ext6) return VG_ERR_ARG;
    if (n_clusters > 0 && (!points || !index || !seg_off)) return VG_ERR_ARG;
    nothing = false;
    return VG_OK;
}

extern "C" int vg_cluster_oriented_extents(const float* d_points, int stride, const int32_t* d_index, const int32_t* d_seg_off, int n_clusters,
                                           const int32_t* d_pair_cluster, int n_pairs, const float* d_center3, const double* d_rot4,
                                           double* d_ext6, void* stream) {
    bool nothing;
    const int rc = oext_check(d_points, stride, d_index, d_seg_off, n_clusters, d_pair_cluster, n_pairs, d_center3, d_rot4, d_ext6, nothing);
    if (rc != VG_OK || nothing) return rc;
    hipLaunchKernelGGL(k_cluster_oriented_extents, dim3((unsigned)n_pairs), dim3(OEXT_BLOCK), 0, (hipStream_t)stream, d_points, stride,
                       d_index, d_seg_off, n_clusters, d_pair_cluster, d_center3, d_rot4, d_ext6);
    VG_LAUNCH_CHECK();
    return VG_OK;
}

extern "C" int vg_cluster_oriented_extents_host(const float* h_points, int stride, const int32_t* h_index, const int32_t* h_seg_off,
                                                int n_clusters, const int32_t* h_pair_cluster, int n_pairs, const float* h_center3,
                                                const double* h_rot4, double* h_ext6) {
    bool nothing;
    const int rc = oext_check(h_points, stride, h_index, h_seg_off, n_clusters, h_pair_cluster, n_pairs, h_center3, h_rot4, h_ext6, nothing);
    if (rc != VG_OK || nothing) return rc;
    for (int64_t p = 0; p < n_pairs; ++p) {
        const int c = h_pair_cluster ? h_pair_cluster[p] : (int)p;
        double* out = h_ext6 + p * 6;
        int64_t lo = 0, hi = 0;
        if (c >= 0 && c < n_clusters) {
            lo = h_seg_off[c];
            hi = h_seg_off[c + 1];
        }
        const float cx = h_center3[p * 3 + 0], cy = h_center3[p * 3 + 1], cz = h_center3[p * 3 + 2];
        OextAcc a;
        a.bad = 1;
        if (hi > lo && oext_finite(cx) && oext_finite(cy) && oext_finite(cz)) {
            const OextRot rot = {h_rot4[p * 4 + 0], h_rot4[p * 4 + 1], h_rot4[p * 4 + 2], h_rot4[p * 4 + 3]};
            double q[3];
            for (int64_t i = lo; i < hi; ++i) {
                const float* r = h_points + (int64_t)h_index[i] * stride;
                const bool ok = oext_point(r[0], r[1], r[2], cx, cy, rot, q);
                if (i == lo) oext_first(a, q, ok);
                else oext_fold(a, q, ok);
            }
        }
        for (int k = 0; k < 6; ++k) out[k] = a.bad ? __builtin_nan("") : a.v[k];
    }
    return VG_OK;
}
