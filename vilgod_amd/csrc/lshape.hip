// L-shape box fits for gfx950: fit_bounding_boxes_simple with method.name = closeness_rectangle / variance_rectangle.
//
//   k_lshape_score     criterion[c, a] of every (cluster, angle) pair, one wave per angle:
//                        0 closeness  pointcloud_utils.py:170-196 check_all_angles: sum_i 1 / max(min(Dx_i, Dy_i), delta_zero) over
//                                     the float32 projection.  The reference runs this function under numba, whose
//                                     np.maximum(float32[:], float) types the Python literal as float64: beta, 1/beta and the sum
//                                     are float64 there, and here (plain NumPy would keep float32)
//                        1 variance   pointcloud_utils.py:231-258: -var(Dx[Dx < Dy]) - var(Dy[Dy < Dx]) over the float64 projection of
//                                     the float32 points; np.var with ddof = 0 as numpy computes it (the mean first, then the sum of
//                                     squared deviations: three passes over the points); a side without points adds nothing
//   k_lshape_pick      per cluster: the FIRST index of the maximum (the reference's strict `>` keeps the earliest angle), the
//                      projection at that angle, + pi/2 when the x extent is the smaller (:206-215, :268-278), the corners (float32
//                      for closeness: its `components` are float32; float64 for variance) and the box of zero_shot_detector.py:452-461
//                      in the dtypes the reference's own expressions give (boxes.box_from_rectangle: l, w, centre float32 for
//                      float32 corners; cz and h + 0.3 float32 from the cluster's float32 z extent)
//
// Products with two terms (`points @ components.T`, `rval @ components`) are rounded as the BLAS gemm behind numpy's dot rounds
// them: the first product rounded, the second added by one FMA (fma(y, s, x * c)); the file is compiled without contraction, so
// these are the only FMAs.  The angle table comes from the host (vilgod_amd/boxes.py lshape_angle_table; layout in
// include/vilgod_hip.h): the angles of np.arange(0, 90 + delta, delta) / 180 * np.pi and the cos / sin the reference evaluates,
// rounded to its component dtype, so no kernel reproduces arange or the host's cos.  Points are read through d_index from global
// memory (L2): clusters of any size work, nothing is staged in LDS.  Min / max start from the cluster's first point, not from a
// float64 infinity (a wave-uniform float64 constant with a non-zero high half can be mis-encoded by the gfx950 back end:
// build.check_isa).
#include <math.h>
#include <type_traits>
#include "common.h"
#include "vilgod_hip.h"

#define LS_WAVES 4            // angles (waves) per block of k_lshape_score

__device__ __forceinline__ float ls_fma(float a, float b, float c) { return fmaf(a, b, c); }
__device__ __forceinline__ double ls_fma(double a, double b, double c) { return fma(a, b, c); }

// [x, y] @ [[c, s], [-s, c]].T (:181-185, :238-243) and [u, v] @ [[c, s], [-s, c]] (:227, :286), rounded like gemm (above)
template <typename T>
__device__ __forceinline__ void ls_proj(T x, T y, T c, T s, T& u, T& v) {
    u = ls_fma(y, s, x * c);
    v = ls_fma(y, c, x * -s);
}
template <typename T>
__device__ __forceinline__ void ls_corner(T u, T v, T c, T s, T& x, T& y) {
    x = ls_fma(v, -s, u * c);
    y = ls_fma(v, c, u * s);
}

// min_axis_zero_2d (:162-167) and np.vstack(...).min(axis=0): the second value unless the first is strictly smaller
template <typename T>
__device__ __forceinline__ T ls_min(T a, T b) { return a < b ? a : b; }

// point i of the cluster that starts at p0, in the criterion's dtype
template <typename T>
__device__ __forceinline__ void ls_point(const float* __restrict__ pts, int stride, const int* __restrict__ index, int p0, int i,
                                         T& x, T& y) {
    const float* p = pts + (size_t)index[p0 + i] * stride;
    x = (T)p[0];
    y = (T)p[1];
}

template <int CRIT>
__global__ __launch_bounds__(256) void k_lshape_score(const float* __restrict__ pts, int stride, const int* __restrict__ index,
                                                      const int* __restrict__ seg_off, const double* __restrict__ table, int n_angles,
                                                      double delta_zero, double* __restrict__ work) {
    typedef typename std::conditional<CRIT == VG_LSHAPE_CLOSENESS, float, double>::type T;
    const int c = blockIdx.x;
    const int a = blockIdx.y * LS_WAVES + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (a >= n_angles) return;                       // whole waves only: this kernel has no block-wide barrier
    const int p0 = seg_off[c], n = seg_off[c + 1] - p0;
    double crit = 0.0;                               // (an empty cluster: empty sums)
    if (n > 0) {
        const double* t = table + (size_t)a * VG_LSHAPE_TABLE_STRIDE;
        const T cs = (T)t[0], sn = (T)t[1];          // exact: a closeness table holds float32 values
        T x, y, u, v;
        ls_point(pts, stride, index, p0, 0, x, y);
        ls_proj(x, y, cs, sn, u, v);
        T mnx = u, mxx = u, mny = v, mxy = v;
        for (int i = lane; i < n; i += WAVE) {
            ls_point(pts, stride, index, p0, i, x, y);
            ls_proj(x, y, cs, sn, u, v);
            mnx = u < mnx ? u : mnx; mxx = u > mxx ? u : mxx; mny = v < mny ? v : mny; mxy = v > mxy ? v : mxy;
        }
        mnx = vg_wave_min(mnx); mxx = vg_wave_max(mxx); mny = vg_wave_min(mny); mxy = vg_wave_max(mxy);
        if (CRIT == VG_LSHAPE_CLOSENESS) {
            double acc = 0.0;
            for (int i = lane; i < n; i += WAVE) {
                ls_point(pts, stride, index, p0, i, x, y);
                ls_proj(x, y, cs, sn, u, v);
                const T dx = ls_min(u - mnx, mxx - u), dy = ls_min(v - mny, mxy - v);
                double beta = (double)ls_min(dx, dy);
                beta = beta < delta_zero ? delta_zero : beta;   // np.maximum(beta, delta_zero), float64
                acc += 1.0 / beta;
            }
            crit = vg_wave_sum(acc);
        } else {
            int nx = 0, ny = 0;
            double sx = 0.0, sy = 0.0;
            for (int i = lane; i < n; i += WAVE) {
                ls_point(pts, stride, index, p0, i, x, y);
                ls_proj(x, y, cs, sn, u, v);
                const double dx = ls_min(u - mnx, mxx - u), dy = ls_min(v - mny, mxy - v);
                if (dx < dy) { nx++; sx += dx; }
                if (dy < dx) { ny++; sy += dy; }
            }
            nx = vg_wave_sum(nx); ny = vg_wave_sum(ny);
            sx = vg_wave_sum(sx); sy = vg_wave_sum(sy);
            const double mx = nx > 0 ? sx / (double)nx : 0.0, my = ny > 0 ? sy / (double)ny : 0.0;
            double qx = 0.0, qy = 0.0;
            for (int i = lane; i < n; i += WAVE) {
                ls_point(pts, stride, index, p0, i, x, y);
                ls_proj(x, y, cs, sn, u, v);
                const double dx = ls_min(u - mnx, mxx - u), dy = ls_min(v - mny, mxy - v);
                if (dx < dy) { const double e = dx - mx; qx += e * e; }
                if (dy < dx) { const double e = dy - my; qy += e * e; }
            }
            qx = vg_wave_sum(qx); qy = vg_wave_sum(qy);
            if (nx > 0) crit += -(qx / (double)nx);
            if (ny > 0) crit += -(qy / (double)ny);
        }
    }
    if (lane == 0) work[(size_t)c * n_angles + a] = crit;
}

// ---------------------------------------------------------------------------------------------
// min / max of the cluster's projection with (cs, sn), over the whole 256-thread block; every thread returns the result
template <typename T>
__device__ void ls_block_extent(const float* __restrict__ pts, int stride, const int* __restrict__ index, int p0, int n, T cs, T sn,
                                T& mnx, T& mxx, T& mny, T& mxy, T (*slot)[4]) {
    const int tid = threadIdx.x;
    T x, y, u, v;
    ls_point(pts, stride, index, p0, 0, x, y);
    ls_proj(x, y, cs, sn, u, v);
    mnx = u; mxx = u; mny = v; mxy = v;
    for (int i = tid; i < n; i += 256) {
        ls_point(pts, stride, index, p0, i, x, y);
        ls_proj(x, y, cs, sn, u, v);
        mnx = u < mnx ? u : mnx; mxx = u > mxx ? u : mxx; mny = v < mny ? v : mny; mxy = v > mxy ? v : mxy;
    }
    __syncthreads();                                 // (the slots may still be read: the z extent, a previous call)
    vg_block_put(slot[0], vg_wave_min(mnx)); vg_block_put(slot[1], vg_wave_max(mxx));
    vg_block_put(slot[2], vg_wave_min(mny)); vg_block_put(slot[3], vg_wave_max(mxy));
    __syncthreads();
    mnx = vg_block_min(slot[0]); mxx = vg_block_max(slot[1]); mny = vg_block_min(slot[2]); mxy = vg_block_max(slot[3]);
}

// box[c] = {cx, cy, cz, l, w, h + 0.3, rz}; aux[c] = {chosen angle index, its criterion, rz before the l/w swap}
template <int CRIT>
__global__ __launch_bounds__(256) void k_lshape_pick(const float* __restrict__ pts, int stride, const int* __restrict__ index,
                                                     const int* __restrict__ seg_off, const double* __restrict__ table, int n_angles,
                                                     const double* __restrict__ work, double* __restrict__ box, double* __restrict__ aux) {
    typedef typename std::conditional<CRIT == VG_LSHAPE_CLOSENESS, float, double>::type T;
    __shared__ union {                               // one phase after the other, a barrier between them
        struct { double v[4]; int i[4]; } best;
        float z[2][4];
        T ext[4][4];
    } red;
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int p0 = seg_off[c], n = seg_off[c + 1] - p0;
    // first index of the maximum: every thread starts from angle 0 and walks its angles upwards with a strict `>`; the threads
    // then combine by (criterion descending, index ascending)
    const double* wc = work + (size_t)c * n_angles;
    double best = wc[0];
    int bi = 0;
    for (int a = tid; a < n_angles; a += 256) {
        const double v = wc[a];
        if (v > best) { best = v; bi = a; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(best, o);
        const int oi = __shfl_xor(bi, o);
        if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
    }
    if (lane == 0) { red.best.v[wv] = best; red.best.i[wv] = bi; }
    __syncthreads();
    best = red.best.v[0]; bi = red.best.i[0];
    for (int k = 1; k < 4; ++k)
        if (red.best.v[k] > best || (red.best.v[k] == best && red.best.i[k] < bi)) { best = red.best.v[k]; bi = red.best.i[k]; }
    if (n == 0) {                                    // nothing to fit: a NaN box (the reference never sees an empty cluster)
        if (tid == 0) {
            const double nan = (double)__int_as_float(0x7fc00000);
            for (int k = 0; k < 7; ++k) box[(size_t)c * 7 + k] = nan;
            aux[(size_t)c * 3 + 0] = (double)bi; aux[(size_t)c * 3 + 1] = best; aux[(size_t)c * 3 + 2] = nan;
        }
        return;                                      // (uniform over the block: no barrier follows for anyone)
    }
    const double* t = table + (size_t)bi * VG_LSHAPE_TABLE_STRIDE;
    // z extent of the cluster, float32
    __syncthreads();                                 // (red was read above)
    const VgExtent e = vg_cluster_extent<1, false>(pts, stride, index + p0, n, nullptr, red.z, nullptr);
    const float zmin = e.lo[2], zmax = e.hi[2];
    // the projection at the chosen angle; the other orientation when its x extent is the smaller (:206-215, :268-278)
    T cs = (T)t[0], sn = (T)t[1];
    T mnx, mxx, mny, mxy;
    ls_block_extent(pts, stride, index, p0, n, cs, sn, mnx, mxx, mny, mxy, red.ext);
    const bool flip = (T)(mxx - mnx) < (T)(mxy - mny);
    if (flip) {
        cs = (T)t[2]; sn = (T)t[3];
        ls_block_extent(pts, stride, index, p0, n, cs, sn, mnx, mxx, mny, mxy, red.ext);
    }
    // corners: rval @ components, rval = [[max_x, min_y], [min_x, min_y], [min_x, max_y], [max_x, max_y]]
    T c0x, c0y, c1x, c1y, c2x, c2y, c3x, c3y;
    ls_corner(mxx, mny, cs, sn, c0x, c0y);
    ls_corner(mnx, mny, cs, sn, c1x, c1y);
    ls_corner(mnx, mxy, cs, sn, c2x, c2y);
    ls_corner(mxx, mxy, cs, sn, c3x, c3y);
    // zero_shot_detector.py:452-461: l = |c0 - c1|, w = |c0 - c3|, centre = (c0 + c2) / 2, all in the corners' dtype
    const T ax = c0x - c1x, ay = c0y - c1y, bx = c0x - c3x, by = c0y - c3y;
    const T l = sqrt(ax * ax + ay * ay), w = sqrt(bx * bx + by * by);
    const bool swap = w > l;
    double out[7];
    out[0] = (double)((c0x + c2x) / (T)2);
    out[1] = (double)((c0y + c2y) / (T)2);
    const float height = zmax - zmin;                // float32 throughout, as the reference's expressions under NumPy 2 promotion
    out[2] = (double)(zmin + height / 2.f);
    out[3] = (double)(swap ? w : l);
    out[4] = (double)(swap ? l : w);
    out[5] = (double)(height + 0.3f);
    // rz: the table's angle (+ pi/2 of the flip), + pi/2 again for the l/w swap -- every sum precomputed on the host in float64
    out[6] = t[4 + (flip ? 1 : 0) + (swap ? 2 : 0)];
    if (tid == 0) {
        for (int k = 0; k < 7; ++k) box[(size_t)c * 7 + k] = out[k];
        aux[(size_t)c * 3 + 0] = (double)bi; aux[(size_t)c * 3 + 1] = best; aux[(size_t)c * 3 + 2] = t[4 + (flip ? 1 : 0)];
    }
}

extern "C" int vg_cluster_lshape(const float* d_points, int stride, const int32_t* d_index, const int32_t* d_seg_off, int n_clusters,
                                 int criterion, const double* d_angle_table, int n_angles, double delta_zero, double* d_work,
                                 double* d_box7, double* d_aux, void* stream) {
    if (criterion != VG_LSHAPE_CLOSENESS && criterion != VG_LSHAPE_VARIANCE) return VG_ERR_ARG;
    if (n_angles < 1 || n_angles > VG_LSHAPE_MAX_ANGLES) return VG_ERR_ARG;
    if (criterion == VG_LSHAPE_CLOSENESS && !(delta_zero > 0)) return VG_ERR_ARG;
    if (n_clusters < 0 || stride < 3) return VG_ERR_ARG;
    if (n_clusters == 0) return VG_OK;
    if (!d_points || !d_index || !d_seg_off || !d_angle_table || !d_work || !d_box7 || !d_aux) return VG_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(n_clusters, vg_div_up(n_angles, LS_WAVES));
    if (criterion == VG_LSHAPE_CLOSENESS) {
        hipLaunchKernelGGL(k_lshape_score<VG_LSHAPE_CLOSENESS>, grid, dim3(WAVE * LS_WAVES), 0, st, d_points, stride, d_index, d_seg_off,
                           d_angle_table, n_angles, delta_zero, d_work);
        hipLaunchKernelGGL(k_lshape_pick<VG_LSHAPE_CLOSENESS>, dim3(n_clusters), dim3(256), 0, st, d_points, stride, d_index, d_seg_off,
                           d_angle_table, n_angles, d_work, d_box7, d_aux);
    } else {
        hipLaunchKernelGGL(k_lshape_score<VG_LSHAPE_VARIANCE>, grid, dim3(WAVE * LS_WAVES), 0, st, d_points, stride, d_index, d_seg_off,
                           d_angle_table, n_angles, delta_zero, d_work);
        hipLaunchKernelGGL(k_lshape_pick<VG_LSHAPE_VARIANCE>, dim3(n_clusters), dim3(256), 0, st, d_points, stride, d_index, d_seg_off,
                           d_angle_table, n_angles, d_work, d_box7, d_aux);
    }
    VG_LAUNCH_CHECK();
    return VG_OK;
}
