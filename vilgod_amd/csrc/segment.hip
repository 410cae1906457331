// Per-cluster reductions for gfx950.
//
//   k_ref_transform    points_ref = T_ref * [p,1] rounded to float32 (lidar_frame.py:66-69, pointcloud_utils.py:21-46)
//   k_plane_hyp/...    C2: ground plane by RANSAC (lidar_frame.py:96-109 -> pointcloud_utils.fit_plane :375-387 ->
//                      pyransac3d Plane.fit): same algorithm, but the three sample indices of every iteration
//                      come from a counter-based hash (seed, iteration) instead of python's `random`
//                      (un-vendored library + global RNG state: PARITY UNPINNED)
//   k_cluster_filter   B4 + C1: per cluster n, z extent, signed plane distances -> the three active validity
//                      filters (cluster_utils.py:14-15, 48-49, 51-60; objects.py:158-181)
//   k_cluster_filter_ex  all seven filters of cluster_utils.py:14-64 (aspect ratio, hull area / volume, score percentile
//                      too) with the and / or / required combination of objects.py:158-181
//   k_cluster_box      E1: 2-D convex hull (gift wrapping with exact float64 orientation tests) + minimum-area
//                      rectangle over the hull edges + the box assembly of zero_shot_detector.py:451-461.
//                      Deviation (documented): ALL hull edges are tried; the reference drops the closing edge of
//                      qhull's vertex cycle (pointcloud_utils.py:329-330), whose start vertex is an artefact of qhull.
#include <string.h>
#include <math.h>
#include "common.h"
#include "vilgod_hip.h"

// ---------------------------------------------------------------------------------------------
__global__ void k_ref_transform(const float* __restrict__ src, int n, int stride, const double* __restrict__ T,
                                float* __restrict__ dst) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* p = src + (size_t)i * stride;
    float* q = dst + (size_t)i * stride;
    double x = p[0], y = p[1], z = p[2];
#pragma unroll
    for (int r = 0; r < 3; ++r) q[r] = (float)(((T[r * 4] * x + T[r * 4 + 1] * y) + T[r * 4 + 2] * z) + T[r * 4 + 3]);
    for (int c = 3; c < stride; ++c) q[c] = p[c];
}

// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long vg_mix64(unsigned long long z) {   // splitmix64 finaliser
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// sample ids of iteration `it`: draw j = 0,1,2,... from the hash stream, skipping repeats (random.sample semantics:
// three distinct indices)
__device__ void vg_sample3(unsigned long long seed, int it, int n, int s[3]) {
    int got = 0;
    for (unsigned int j = 0; got < 3; ++j) {
        unsigned long long h = vg_mix64(seed * 0x100000001B3ull + ((unsigned long long)it << 20) + j);
        int v = (int)(h % (unsigned long long)n);
        bool dup = false;
        for (int t = 0; t < got; ++t) dup |= (s[t] == v);
        if (!dup) s[got++] = v;
    }
}

// one block per hypothesis.  idx: optional index list into pts (NULL = identity).  plane_out[it] = {a,b,c,d}, count_out[it]
__global__ __launch_bounds__(256) void k_plane_hyp(const float* __restrict__ pts, int stride, const int* __restrict__ idx,
                                                   int n, double thresh, unsigned long long seed,
                                                   double* __restrict__ plane_out, int* __restrict__ count_out) {
    __shared__ double pl[4];
    __shared__ int cnt[4];
    // grid = (iterations, PLANE_SPLIT): the inlier count of a hypothesis is summed over PLANE_SPLIT blocks (integer atomics into the
    // zeroed count array: exact, order-free) -- 100 blocks alone leave more than half of the 256 CUs idle for ~140 us
    const int it = blockIdx.x, part = blockIdx.y, nparts = gridDim.y;
    if (threadIdx.x == 0) {
        int s[3];
        vg_sample3(seed, it, n, s);
        double P[3][3];
        for (int t = 0; t < 3; ++t) {
            const float* p = pts + (size_t)(idx ? idx[s[t]] : s[t]) * stride;
            P[t][0] = p[0]; P[t][1] = p[1]; P[t][2] = p[2];
        }
        double A[3] = {P[1][0] - P[0][0], P[1][1] - P[0][1], P[1][2] - P[0][2]};
        double B[3] = {P[2][0] - P[0][0], P[2][1] - P[0][1], P[2][2] - P[0][2]};
        double C[3] = {A[1] * B[2] - A[2] * B[1], A[2] * B[0] - A[0] * B[2], A[0] * B[1] - A[1] * B[0]};
        double nrm = sqrt((C[0] * C[0] + C[1] * C[1]) + C[2] * C[2]);
        C[0] /= nrm; C[1] /= nrm; C[2] /= nrm;
        pl[0] = C[0]; pl[1] = C[1]; pl[2] = C[2];
        pl[3] = -((C[0] * P[1][0] + C[1] * P[1][1]) + C[2] * P[1][2]);
    }
    __syncthreads();
    const double plane[4] = {pl[0], pl[1], pl[2], pl[3]};
    const double inv = vg_plane_norm(plane);
    int local = 0;
    for (int i = part * 256 + threadIdx.x; i < n; i += 256 * nparts) {
        const float* p = pts + (size_t)(idx ? idx[i] : i) * stride;
        if (fabs(vg_plane_distance(plane, inv, p)) <= thresh) local++;
    }
    vg_block_put(cnt, vg_wave_sum(local));
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicAdd(&count_out[it], vg_block_sum(cnt));
        if (part == 0)
            for (int k = 0; k < 4; ++k) plane_out[it * 4 + k] = pl[k];
    }
}

// first hypothesis with the strictly largest inlier count (pyransac3d keeps the first best); writes best plane
__global__ void k_plane_best(const double* __restrict__ planes, const int* __restrict__ counts, int iters,
                             double* __restrict__ best_plane, int* __restrict__ best_count) {
    if (threadIdx.x != 0) return;
    int b = -1, bc = 0;
    for (int i = 0; i < iters; ++i)
        if (counts[i] > bc) { bc = counts[i]; b = i; }
    for (int k = 0; k < 4; ++k) best_plane[k] = b >= 0 ? planes[b * 4 + k] : 0.0;
    best_count[0] = bc;
}

__global__ void k_plane_inliers(const float* __restrict__ pts, int stride, const int* __restrict__ idx, int n,
                                const double* __restrict__ plane, double thresh, unsigned char* __restrict__ flags) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* p = pts + (size_t)(idx ? idx[i] : i) * stride;
    flags[i] = fabs(vg_plane_distance(plane, vg_plane_norm(plane), p)) <= thresh ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------
// The three shipped filters from a cluster's point count, float32 height (objects.py:112-114) and plane-distance extremes.
struct VgShippedVerdicts { bool number_points, height, plane_distance; };
__device__ __forceinline__ VgShippedVerdicts vg_shipped_verdicts(int n, float height, double dmin, double dmax, int min_points,
                                                                 int max_points, double min_height, double max_height,
                                                                 double max_min_height, double min_max_height) {
    VgShippedVerdicts v;
    v.number_points = n >= min_points && n <= max_points;                              // cluster_utils.py:14-15
    v.height = (double)height >= min_height && (double)height <= max_height;           // :48-49
    v.plane_distance = dmin <= max_min_height && dmax >= min_max_height;               // :58-60
    return v;
}

// stats[c] = {n, zmin, zmax, dmin, dmax, height}; valid[c] per the three active, required, `and` filters.
__global__ __launch_bounds__(256) void k_cluster_filter(const float* __restrict__ pts, int stride,
                                                        const int* __restrict__ index, const int* __restrict__ seg_off,
                                                        const double* __restrict__ plane, int min_points, int max_points,
                                                        double max_min_height, double min_max_height, double min_height,
                                                        double max_height, float* __restrict__ stats,
                                                        unsigned char* __restrict__ valid) {
    __shared__ float rz[2][4];
    __shared__ double rd[2][4];
    const int c = blockIdx.x;
    const int p0 = seg_off[c], n = seg_off[c + 1] - p0;
    const VgExtent e = vg_cluster_extent<1, true>(pts, stride, index + p0, n, plane, rz, rd);
    if (threadIdx.x == 0) {
        const float height = e.hi[2] - e.lo[2];
        const VgShippedVerdicts v = vg_shipped_verdicts(n, height, e.dmin, e.dmax, min_points, max_points, min_height, max_height,
                                                        max_min_height, min_max_height);
        valid[c] = (v.number_points && v.plane_distance && v.height) ? 1 : 0;
        float* s = stats + (size_t)c * 6;
        s[0] = (float)n; s[1] = e.lo[2]; s[2] = e.hi[2]; s[3] = (float)e.dmin; s[4] = (float)e.dmax; s[5] = height;
    }
}

// ---------------------------------------------------------------------------------------------
#define BOX_MAX_HULL VG_BOX_MAX_HULL
// Sign of the orientation of (a,b,c), exact for float32 inputs whose four differences are exact in float64: coordinates within 2^29
// of each other in magnitude (any LiDAR cluster: 2^-20 m .. 2^9 m).  The two products need up to 2 x 53 bits, so their rounded
// difference can have the wrong sign in a cluster that straddles an axis (coordinates from 2^-20 to 2^2 around a near-collinear
// triple).  Where the rounded value is not safely away from zero, the products are split error-free (p + e = d1 * d2 with one fma)
// and (p1 + e1) - (p2 + e2) is summed into a non-overlapping expansion (Shewchuk's Two-Two-Diff): its leading nonzero term has
// the exact sign.  Only the sign and zero-ness of the result are meaningful.
__device__ __forceinline__ void vg_two_sum(double a, double b, double& x, double& y) {
    x = a + b;
    const double bv = x - a, av = x - bv;
    y = (a - av) + (b - bv);
}
__device__ __forceinline__ void vg_two_diff(double a, double b, double& x, double& y) {
    x = a - b;
    const double bv = a - x, av = x + bv;
    y = (a - av) + (bv - b);
}
__device__ __noinline__ double vg_orient_exact(double d1, double d2, double d3, double d4, double p1, double p2) {
    const double e1 = fma(d1, d2, -p1), e2 = fma(d3, d4, -p2);
    double i, j, t, x0, x1, x2, x3;
    vg_two_diff(e1, e2, i, x0);            // (p1, e1) - e2 -> (j, t, x0)
    vg_two_sum(p1, i, j, t);
    vg_two_diff(t, p2, i, x1);             // (j, t) - p2 -> (x3, x2, x1)
    vg_two_sum(j, i, x3, x2);
    return x3 != 0 ? x3 : x2 != 0 ? x2 : x1 != 0 ? x1 : x0;
}
__device__ __forceinline__ double vg_orient(double ax, double ay, double bx, double by, double cx, double cy) {
    const double d1 = bx - ax, d2 = cy - ay, d3 = by - ay, d4 = cx - ax;
    const double p1 = d1 * d2, p2 = d3 * d4;
    const double det = p1 - p2;
    // |det - exact| <= 2^-53 (|p1| + |p2|) + 2^-53 |p1 - p2|: beyond 2^-51 (|p1| + |p2|) the rounded sign is the exact one
    if (fabs(det) > 0x1p-51 * (fabs(p1) + fabs(p2))) return det;
    return vg_orient_exact(d1, d2, d3, d4, p1, p2);
}

// true when candidate o replaces the current best b as the next counter-clockwise vertex seen from (cx0, cy0): no point to its
// right; on a line the farthest, then the lowest position.  The ONLY statement of the rule: thread loop, wave and block combine
__device__ __forceinline__ bool vg_hull_better(double cx0, double cy0, int bi, double bx, double by, double bd2,
                                               int oi, double ox, double oy, double od2) {
    if (oi < 0) return false;
    if (bi < 0) return true;
    const double orr = vg_orient(cx0, cy0, bx, by, ox, oy);
    return orr < 0 || (orr == 0 && (od2 > bd2 || (od2 == bd2 && oi < bi)));
}
// true when point o replaces b as the start vertex: lowest y, then lowest x, then lowest position in the list
__device__ __forceinline__ bool vg_hull_lower(int bi, double bx, double by, int oi, double ox, double oy) {
    // (`&`, `|`: no branches, so the unrolled start pass keeps its gathers in flight)
    return (oi >= 0) & ((bi < 0) | (oy < by) | ((oy == by) & ((ox < bx) | ((ox == bx) & (oi < bi)))));
}

// Convex hull of the xy of one cluster (points pts[idx[i] * stride], i < n) by gift wrapping with exact orientation tests, called
// by a 256-thread workgroup: counter-clockwise from the start vertex, strict vertices only (duplicates and points inside an edge
// are none).  hx / hy [CAP] and s are the caller's LDS; s must be free on entry and is free on return (a barrier ends the walk).
//   n         strict vertices written to hx / hy (<= CAP), uniform over the workgroup
//   overflow  the hull has more than CAP vertices: hx / hy hold the first CAP from the start vertex, the outline is not closed
//             (a hull of exactly CAP vertices closes unflagged)
//   degenerate  fewer than 3 strict vertices: no point, identical or collinear points
struct VgHullLds { double x[4], y[4], d2[4]; int i[4]; int cur; };      // the four waves' candidates; the vertex the walk stands on
struct VgHull { int n; bool degenerate, overflow; };
#define HULL_BATCH 4
template <int CAP>
__device__ __forceinline__ VgHull vg_hull_wrap(const float* __restrict__ pts, int stride, const int* __restrict__ idx, int n,
                                               double* hx, double* hy, VgHullLds& s) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    auto px = [&](int i) { return (double)pts[(size_t)idx[i] * stride]; };
    auto py = [&](int i) { return (double)pts[(size_t)idx[i] * stride + 1]; };
    VgHull h = {0, false, false};
    {
        int bi = -1;
        double bx = 0, by = 0;
#pragma unroll 4                                   // (four gathers in flight)
        for (int i = tid; i < n; i += 256) {
            const double x = px(i), y = py(i);
            if (vg_hull_lower(bi, bx, by, i, x, y)) { bi = i; bx = x; by = y; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const int oi = __shfl_xor(bi, o);
            const double ox = __shfl_xor(bx, o), oy = __shfl_xor(by, o);
            if (vg_hull_lower(bi, bx, by, oi, ox, oy)) { bi = oi; bx = ox; by = oy; }
        }
        if (lane == 0) { s.i[wv] = bi; s.x[wv] = bx; s.y[wv] = by; }
        __syncthreads();
        if (tid == 0) {
            for (int k = 1; k < 4; ++k)
                if (vg_hull_lower(bi, bx, by, s.i[k], s.x[k], s.y[k])) { bi = s.i[k]; bx = s.x[k]; by = s.y[k]; }
            s.cur = bi;
        }
        __syncthreads();
    }
    const int start = s.cur;
    const bool none = start < 0;                                           // (no point: nothing to wrap)
    const double sx0 = none ? 0.0 : px(start), sy0 = none ? 0.0 : py(start);
    while (!none) {
        const int cur = s.cur;
        const double cx0 = px(cur), cy0 = py(cur);
        // capacity: the vertices so far are the first CAP counter-clockwise from the start, the rest of the outline is missing
        if (h.n >= CAP) { h.overflow = true; break; }                      // uniform: h.n is counted by every thread, so the exit
        if (tid == 0) { hx[h.n] = cx0; hy[h.n] = cy0; }                    // never reads a counter that thread 0 is advancing
        h.n++;
        int best = -1;
        double bxx = 0, byy = 0, bd2 = -1;
        // the gathers of HULL_BATCH points are issued before the first of them is judged: the scan waits on memory, not on arithmetic
        for (int i0 = tid; i0 < n; i0 += 256 * HULL_BATCH) {
            double x[HULL_BATCH], y[HULL_BATCH];
#pragma unroll
            for (int u = 0; u < HULL_BATCH; ++u) {
                const int i = i0 + 256 * u < n ? i0 + 256 * u : cur;       // (past the end: the current vertex, which is skipped)
                x[u] = px(i);
                y[u] = py(i);
            }
#pragma unroll
            for (int u = 0; u < HULL_BATCH; ++u) {
                if (x[u] == cx0 && y[u] == cy0) continue;                  // the current vertex itself and its duplicates
                const double d2 = (x[u] - cx0) * (x[u] - cx0) + (y[u] - cy0) * (y[u] - cy0);
                if (vg_hull_better(cx0, cy0, best, bxx, byy, bd2, i0 + 256 * u, x[u], y[u], d2)) {
                    best = i0 + 256 * u; bxx = x[u]; byy = y[u]; bd2 = d2;
                }
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const int oi = __shfl_xor(best, o);
            const double ox = __shfl_xor(bxx, o), oy = __shfl_xor(byy, o), od = __shfl_xor(bd2, o);
            if (vg_hull_better(cx0, cy0, best, bxx, byy, bd2, oi, ox, oy, od)) { best = oi; bxx = ox; byy = oy; bd2 = od; }
        }
        __syncthreads();                                                   // every thread has read s.cur
        if (lane == 0) { s.i[wv] = best; s.x[wv] = bxx; s.y[wv] = byy; s.d2[wv] = bd2; }
        __syncthreads();
        if (tid == 0) {
            for (int k = 1; k < 4; ++k)
                if (vg_hull_better(cx0, cy0, best, bxx, byy, bd2, s.i[k], s.x[k], s.y[k], s.d2[k])) {
                    best = s.i[k]; bxx = s.x[k]; byy = s.y[k]; bd2 = s.d2[k];
                }
            s.cur = best;
        }
        __syncthreads();
        const int nxt = s.cur;
        if (nxt < 0) break;                                                // all points coincide: one vertex
        if (px(nxt) == sx0 && py(nxt) == sy0) break;                       // closed
    }
    __syncthreads();                                                       // hx / hy of the last vertex are visible
    h.degenerate = h.n < 3;
    return h;
}

// box[c] = {cx, cy, cz, l, w, h, rz} (float64, ref frame); aux[c] = {n_hull, area, flag}: flag 0 = a rectangle over the whole hull,
// VG_BOX_FLAG_DEGENERATE = fewer than 3 strict hull vertices (0.1 m square at the mean), VG_BOX_FLAG_HULL_OVERFLOW = the hull has
// more than BOX_MAX_HULL vertices: NO rectangle is fitted (cx, cy, l, w, rz = NaN; cz, h valid), the caller fits that cluster itself
__global__ __launch_bounds__(256) void k_cluster_box(const float* __restrict__ pts, int stride,
                                                     const int* __restrict__ index, const int* __restrict__ seg_off,
                                                     double* __restrict__ box, float* __restrict__ aux) {
    __shared__ double hx[BOX_MAX_HULL], hy[BOX_MAX_HULL];
    __shared__ double ang[BOX_MAX_HULL];
    __shared__ union { VgHullLds hull; float z[2][4]; } sh;              // the z extent is done before the hull starts
    double* const red_v = sh.hull.x;                                      // after the hull: two block-reduction slots
    double* const red_d = sh.hull.y;
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int p0 = seg_off[c], n = seg_off[c + 1] - p0;
    const int* idx = index + p0;
    const VgExtent e = vg_cluster_extent<1, false>(pts, stride, idx, n, nullptr, sh.z, nullptr);
    const float zmin = e.lo[2], zmax = e.hi[2];
    __syncthreads();                                                      // every thread has read sh.z
    // fewer than 3 strict vertices = collinear or identical input (qhull raises -> the reference falls back to a 0.1 m square); three
    // or more have area, the orientation test being exact.  Beyond capacity a rectangle over the stored vertices would cover part of
    // the object, so none is fitted
    const VgHull hull = vg_hull_wrap<BOX_MAX_HULL>(pts, stride, idx, n, hx, hy, sh.hull);
    const int nh = hull.n;
    double out[7];
    float n_hull = (float)nh, area = 0.f, deg = 0.f;
    const float height = zmax - zmin;                                   // zero_shot_detector.py:459 (float32)
    if (hull.overflow) {
        deg = (float)VG_BOX_FLAG_HULL_OVERFLOW;
        out[0] = out[1] = out[3] = out[4] = out[6] = NAN;
    } else if (hull.degenerate) {
        // pointcloud_utils.py:322-326: 0.1 m square at the mean, rz = 0
        deg = (float)VG_BOX_FLAG_DEGENERATE;
        double sx = 0, sy = 0;
        for (int i = tid; i < n; i += 256) {
            sx += (double)pts[(size_t)idx[i] * stride];
            sy += (double)pts[(size_t)idx[i] * stride + 1];
        }
        vg_block_put(red_v, vg_wave_sum(sx));
        vg_block_put(red_d, vg_wave_sum(sy));
        __syncthreads();
        double mx = vg_block_sum(red_v) / (double)n, my = vg_block_sum(red_d) / (double)n;
        out[0] = mx; out[1] = my; out[3] = 0.1; out[4] = 0.1; out[6] = 0.0;
        // corners (-.05,-.05),(.05,-.05),(.05,.05),(-.05,.05): l = |c0-c1| = 0.1, w = |c0-c3| = 0.1
    } else {
        // edge angles mod pi/2, all edges (closing one included)
        for (int i = tid; i < nh; i += 256) {
            int j = (i + 1) % nh;
            double a = atan2(hy[j] - hy[i], hx[j] - hx[i]);
            double m = fmod(a, M_PI / 2.);
            if (m < 0) m += M_PI / 2.;                                   // np.mod semantics (result has the sign of the divisor)
            ang[i] = fabs(m);
        }
        __syncthreads();
        // np.unique: ascending, first minimum wins -> evaluate every angle, keep (area, angle) lexicographic minimum
        double barea = INFINITY, bang = INFINITY;
        for (int i = tid; i < nh; i += 256) {
            const double a = ang[i];
            const double r00 = cos(a), r01 = cos(a - M_PI / 2.), r10 = cos(a + M_PI / 2.), r11 = cos(a);
            double mnx = INFINITY, mxx = -INFINITY, mny = INFINITY, mxy = -INFINITY;
            for (int k = 0; k < nh; ++k) {
                double x = r00 * hx[k] + r01 * hy[k], y = r10 * hx[k] + r11 * hy[k];
                mnx = fmin(mnx, x); mxx = fmax(mxx, x); mny = fmin(mny, y); mxy = fmax(mxy, y);
            }
            double ar = (mxx - mnx) * (mxy - mny);
            if (ar < barea || (ar == barea && a < bang)) { barea = ar; bang = a; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            double oa = __shfl_xor(barea, o), og = __shfl_xor(bang, o);
            if (oa < barea || (oa == barea && og < bang)) { barea = oa; bang = og; }
        }
        if (lane == 0) { red_v[wv] = barea; red_d[wv] = bang; }
        __syncthreads();
        barea = red_v[0]; bang = red_d[0];
        for (int k = 1; k < 4; ++k)
            if (red_v[k] < barea || (red_v[k] == barea && red_d[k] < bang)) { barea = red_v[k]; bang = red_d[k]; }
        // corners (pointcloud_utils.py:359-370) and the box of zero_shot_detector.py:452-461
        const double a = bang;
        const double r00 = cos(a), r01 = cos(a - M_PI / 2.), r10 = cos(a + M_PI / 2.), r11 = cos(a);
        double mnx = INFINITY, mxx = -INFINITY, mny = INFINITY, mxy = -INFINITY;
        for (int k = 0; k < nh; ++k) {
            double x = r00 * hx[k] + r01 * hy[k], y = r10 * hx[k] + r11 * hy[k];
            mnx = fmin(mnx, x); mxx = fmax(mxx, x); mny = fmin(mny, y); mxy = fmax(mxy, y);
        }
        // rval[k] = [u, v] @ r  ->  (u*r00 + v*r10, u*r01 + v*r11)
        const double c0x = mxx * r00 + mny * r10, c0y = mxx * r01 + mny * r11;
        const double c1x = mnx * r00 + mny * r10, c1y = mnx * r01 + mny * r11;
        const double c2x = mnx * r00 + mxy * r10, c2y = mnx * r01 + mxy * r11;
        const double c3x = mxx * r00 + mxy * r10, c3y = mxx * r01 + mxy * r11;
        double l = sqrt((c0x - c1x) * (c0x - c1x) + (c0y - c1y) * (c0y - c1y));
        double w = sqrt((c0x - c3x) * (c0x - c3x) + (c0y - c3y) * (c0y - c3y));
        double rz = a;
        if (w > l) { double t = l; l = w; w = t; rz += M_PI / 2; }
        out[0] = (c0x + c2x) / 2; out[1] = (c0y + c2y) / 2; out[3] = l; out[4] = w; out[6] = rz;
        area = (float)barea;
    }
    out[2] = (double)zmin + (double)height / 2;
    out[5] = (double)height + 0.3;
    if (tid == 0) {
        for (int k = 0; k < 7; ++k) box[(size_t)c * 7 + k] = out[k];
        aux[c * 3 + 0] = n_hull; aux[c * 3 + 1] = area; aux[c * 3 + 2] = deg;
    }
}

// ---------------------------------------------------------------------------------------------
// entropy (PP) score of a query frame from its neighbour counts; numpy's pairwise summation order
// (n < 8: left to right; otherwise 8 running partial sums over blocks of 8, combined as a tree, then the tail).
__device__ double vg_np_pairwise(const double* v, int n) {
    if (n < 8) {
        double s = 0.0;
        for (int i = 0; i < n; ++i) s += v[i];
        return s;
    }
    double r[8];
    for (int j = 0; j < 8; ++j) r[j] = v[j];
    int i = 8;
    for (; i < n - (n % 8); i += 8)
        for (int j = 0; j < 8; ++j) r[j] += v[i + j];
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += v[i];
    return res;
}

__global__ void k_entropy_scores(const int* __restrict__ counts, int nf, int nq, int seek_row, double* __restrict__ H) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    double c[128], t[128];
    long long tot = 0;
    for (int f = 0; f < nf; ++f) {
        int v = counts[(size_t)f * nq + i];
        if (f == seek_row) v -= 1;
        c[f] = (double)v;
        tot += v;
    }
    const double den = (double)tot + 1e-8;
    for (int f = 0; f < nf; ++f) {
        const double P = c[f] / den;
        t[f] = -P * log(P + 1e-8);
    }
    H[i] = vg_np_pairwise(t, nf) / log((double)nf);
}

__global__ void k_subsample_keys(unsigned long long seed, unsigned long long tag, int n, long long* __restrict__ keys) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    keys[i] = (long long)(vg_mix64(seed * 0x100000001B3ull + (tag << 32) + (unsigned long long)i) >> 1);
}

// ---------------------------------------------------------------------------------------------
// Detection.cluster_mass_center = np.median(cluster_points, axis=0) (objects.py:121-123) for every packed cluster
// and the first n_cols columns of the point rows: exact order statistics by a 4-pass byte radix select per (cluster, column);
// an even count gives the float32 mean of the two middle values, like np.median on a float32 array.
// Round 4 (the kernel took 3 ms per frame in the entry point's trace: one workgroup per cluster walked its five columns one after the
// other, every pass gathered the column again from global memory, and the coordinates of one cluster share their leading bytes, so
// 256 threads added to ONE histogram bin with one LDS atomic each): a workgroup per (cluster, column); the column's keys are staged
// in LDS once (<= MED_CAP points; larger clusters keep gathering); the select (common.h) adds to a bin once per wave.
#define MED_CAP 12288
__global__ __launch_bounds__(256) void k_cluster_medians(const float* __restrict__ pts, int stride, int n_cols,
                                                         const int* __restrict__ index, const int* __restrict__ seg_off,
                                                         float* __restrict__ out) {
    __shared__ uint32_t hist[256];
    __shared__ uint32_t sh[6];
    __shared__ uint32_t keys[MED_CAP];
    const int c = blockIdx.x, col = blockIdx.y, t = threadIdx.x;
    const int p0 = seg_off[c], n = seg_off[c + 1] - p0;
    const int* idx = index + p0;
    const auto gathered = [&](int i) { return vg_fkey(pts[(size_t)idx[i] * stride + col]); };
    float m = 0.f;
    if (n > MED_CAP) {
        m = vg_median_select<true>(gathered, n, hist, sh, t);
    } else if (n > 0) {
        for (int i = t; i < n; i += 256) keys[i] = gathered(i);
        __syncthreads();
        m = vg_median_select<true>([&](int i) { return keys[i]; }, n, hist, sh, t);
    }
    if (t == 0) out[(size_t)c * n_cols + col] = m;
}

// ---------------------------------------------------------------------------------------------
// Every filter of cluster_utils.py with Detection.filter's and / or / required combination (objects.py:158-181).
// One workgroup per cluster, walking a persistent grid.  Per cluster: the extent pass of k_cluster_filter with x and y added,
// vg_hull_wrap for the xy hull (only when area or volume is active), a radix select on the scores (only when the ephemeral filter
// is active).  The hull's vertices and the select's staged keys share one LDS buffer: the two phases do not overlap.
#define FEX_HULL_CAP 1024
#define FEX_KEY_CAP 4096
__global__ __launch_bounds__(256) void k_cluster_filter_ex(const float* __restrict__ pts, int stride,
                                                           const int* __restrict__ index, const int* __restrict__ seg_off,
                                                           int n_clusters, const double* __restrict__ plane,
                                                           const float* __restrict__ scores, const vg_filter_params P,
                                                           double* __restrict__ stats, unsigned char* __restrict__ verdict,
                                                           unsigned char* __restrict__ valid) {
    __shared__ double buf[2 * FEX_HULL_CAP];            // hx | hy, or FEX_KEY_CAP staged keys
    __shared__ uint32_t hist[256];
    __shared__ uint32_t sel[6];
    __shared__ union { VgHullLds hull; struct { float f[6][4]; double d[2][4]; } ext; } red;   // the extent is done before the hull starts
    double* hx = buf;
    double* hy = buf + FEX_HULL_CAP;
    uint32_t* keys = reinterpret_cast<uint32_t*>(buf);
    const int tid = threadIdx.x;
    const bool want_hull = P.active[VG_FILTER_AREA] || P.active[VG_FILTER_VOLUME];
    const bool want_q = P.active[VG_FILTER_EPHEMERAL_SCORE] != 0;
    for (int c = blockIdx.x; c < n_clusters; c += gridDim.x) {
        const int p0 = seg_off[c], n = seg_off[c + 1] - p0;
        const int* idx = index + p0;
        const VgExtent e = vg_cluster_extent<3, true>(pts, stride, idx, n, plane, red.ext.f, red.ext.d);
        const float height = e.hi[2] - e.lo[2];

        // ---- convex hull of xy (cluster_utils.py:25-46) ----
        VgHull hull = {0, false, false};
        double area = 0.0, abs_sum = 0.0;
        if (want_hull && n >= 3) {
            __syncthreads();                                               // every thread has read red.ext
            hull = vg_hull_wrap<FEX_HULL_CAP>(pts, stride, idx, n, hx, hy, red.hull);
            if (hull.n >= 2 && !hull.overflow) {
                // shoelace in float64 (products of float32 values are exact); every thread computes the same serial sum.  A closed
                // 2-vertex walk (collinear points) has two edges for abs_sum and an area of exactly 0
                double a2 = 0.0;
                for (int i = 0; i < hull.n; ++i) {
                    const int j = i + 1 == hull.n ? 0 : i + 1;
                    const double t0 = hx[i] * hy[j], t1 = hx[j] * hy[i];
                    a2 += t0 - t1;
                    abs_sum += fabs(t0) + fabs(t1);
                }
                area = 0.5 * fabs(a2);
                if (!(area > 0.0)) { hull.degenerate = true; area = 0.0; }
            }
        }
        const double volume = area * (double)height;                       // cluster_utils.py:30 (float64 here)

        // ---- percentile of the scores (cluster_utils.py:62-64; numpy's linear method) ----
        double q = 0.0;
        if (want_q && n > 0) {
            __syncthreads();                                               // the hull buffer becomes the key buffer
            const double virt = (P.percentile / 100.0) * (double)(n - 1);
            int lo = (int)floor(virt);
            lo = lo < 0 ? 0 : (lo > n - 1 ? n - 1 : lo);
            const double g = virt - (double)lo;
            const int hi = lo + 1 < n ? lo + 1 : n - 1;
            const auto gathered = [&](int i) { return vg_fkey(scores[idx[i]]); };
            float va, vb;
            if (n <= FEX_KEY_CAP) {
                for (int i = tid; i < n; i += 256) keys[i] = gathered(i);
                __syncthreads();
                const auto staged = [&](int i) { return keys[i]; };
                va = vg_radix_select<true>(staged, n, lo, hist, sel, tid);
                vb = hi == lo ? va : vg_radix_select<true>(staged, n, hi, hist, sel, tid);
            } else {
                va = vg_radix_select<true>(gathered, n, lo, hist, sel, tid);
                vb = hi == lo ? va : vg_radix_select<true>(gathered, n, hi, hist, sel, tid);
            }
            const double A = (double)va, B = (double)vb, dd = B - A;
            q = g >= 0.5 ? B - dd * (1.0 - g) : A + dd * g;               // frame_state.static_from_entropy
        }

        if (tid == 0) {
            unsigned char v[VG_FILTER_COUNT];
            const VgShippedVerdicts sv = vg_shipped_verdicts(n, height, e.dmin, e.dmax, P.min_points, P.max_points, P.min_height,
                                                             P.max_height, P.max_min_height, P.min_max_height);
            v[VG_FILTER_NUMBER_POINTS] = sv.number_points;
            v[VG_FILTER_HEIGHT] = sv.height;
            v[VG_FILTER_PLANE_DISTANCE] = sv.plane_distance;
            const float sx = e.hi[0] - e.lo[0], sy = e.hi[1] - e.lo[1];                                    // :18 (float32)
            const float ratio = fmaxf(sx, sy) / fminf(sx, sy);                                             // :20 (x/0 = inf, 0/0 = nan)
            v[VG_FILTER_ASPECT_RATIO] = (((double)ratio >= P.min_aspect_ratio) || sx < 1.0f || sy < 1.0f) &&
                                        ((double)ratio <= P.max_aspect_ratio);                             // :20-23
            bool okv = n >= 3 && !hull.overflow && volume >= P.min_volume;                                 // :26-34
            if (P.has_max_volume) okv = okv && volume <= P.max_volume;
            bool oka = n >= 3 && !hull.overflow && area >= P.min_area;                                     // :37-46
            if (P.has_max_area) oka = oka && area <= P.max_area;
            v[VG_FILTER_VOLUME] = okv;
            v[VG_FILTER_AREA] = oka;
            v[VG_FILTER_EPHEMERAL_SCORE] = !(q > P.min_percentile_pp_score);                               // :64
            // objects.py:181: (all(and) or any(or)) and all(and_required); all([]) = True, any([]) = False
            bool all_and = true, any_or = false, all_req = true;
            for (int k = 0; k < VG_FILTER_COUNT; ++k) {
                if (!P.active[k]) { v[k] = 0; continue; }
                if (P.logic[k] == VG_FILTER_AND_REQUIRED) all_req = all_req && v[k];
                else if (P.logic[k] == VG_FILTER_AND) all_and = all_and && v[k];
                else any_or = any_or || v[k];
            }
            for (int k = 0; k < VG_FILTER_COUNT; ++k) verdict[(size_t)c * VG_FILTER_COUNT + k] = v[k];
            valid[c] = ((all_and || any_or) && all_req) ? 1 : 0;
            double* s = stats + (size_t)c * VG_FILTER_NSTATS;
            s[0] = (double)n; s[1] = (double)e.lo[2]; s[2] = (double)e.hi[2]; s[3] = e.dmin; s[4] = e.dmax; s[5] = (double)height;
            s[6] = (double)sx; s[7] = (double)sy; s[8] = (double)ratio; s[9] = area; s[10] = volume; s[11] = (double)hull.n;
            s[12] = (double)((hull.degenerate ? VG_FILTER_FLAG_DEGENERATE : 0) | (hull.overflow ? VG_FILTER_FLAG_HULL_OVERFLOW : 0));
            s[13] = q; s[14] = abs_sum; s[15] = 0.0;
        }
        __syncthreads();                                                   // the next cluster reuses every shared array
    }
}

extern "C" {

int vg_cluster_medians(const float* d_points, int stride, int n_cols, const int32_t* d_index, const int32_t* d_seg_off, int n_clusters,
                       float* d_median, void* stream) {
    if (n_clusters <= 0) return VG_OK;
    if (!d_points || !d_index || !d_seg_off || !d_median || n_cols <= 0 || n_cols > stride) return VG_ERR_ARG;
    hipLaunchKernelGGL(k_cluster_medians, dim3(n_clusters, n_cols), dim3(256), 0, (hipStream_t)stream, d_points, stride, n_cols, d_index, d_seg_off,
                       d_median);
    VG_LAUNCH_CHECK();
    return VG_OK;
}

int vg_ref_transform(const float* d_src, int n, int stride, const double* d_T4x4, float* d_dst, void* stream) {
    if (n <= 0) return VG_OK;
    if (!d_src || !d_dst || !d_T4x4 || stride < 3) return VG_ERR_ARG;
    hipLaunchKernelGGL(k_ref_transform, dim3(vg_div_up(n, 256)), dim3(256), 0, (hipStream_t)stream, d_src, n, stride, d_T4x4, d_dst);
    VG_LAUNCH_CHECK();
    return VG_OK;
}

/* d_work: >= iters*(4*8+4) + 64 bytes of scratch.  d_plane4: best plane {a,b,c,d} (f64).  d_flags: [n] inlier flags of it.
 * d_count: [1] inlier count. */
int vg_plane_ransac(const float* d_points, int stride, const int32_t* d_index, int n, double thresh, int iters,
                    uint64_t seed, void* d_work, double* d_plane4, uint8_t* d_flags, int32_t* d_count, void* stream) {
    if (!d_points || !d_work || !d_plane4 || !d_flags || !d_count || iters <= 0 || stride < 3) return VG_ERR_ARG;
    if (n < 3) return VG_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    double* planes = (double*)d_work;
    int* counts = (int*)((char*)d_work + (size_t)iters * 32);
    VG_CHECK(hipMemsetAsync(counts, 0, sizeof(int) * (size_t)iters, st));
    hipLaunchKernelGGL(k_plane_hyp, dim3(iters, 4), dim3(256), 0, st, d_points, stride, d_index, n, thresh,
                       (unsigned long long)seed, planes, counts);
    hipLaunchKernelGGL(k_plane_best, dim3(1), dim3(64), 0, st, planes, counts, iters, d_plane4, d_count);
    hipLaunchKernelGGL(k_plane_inliers, dim3(vg_div_up(n, 256)), dim3(256), 0, st, d_points, stride, d_index, n, d_plane4, thresh, d_flags);
    VG_LAUNCH_CHECK();
    return VG_OK;
}

int vg_cluster_filter(const float* d_points, int stride, const int32_t* d_index, const int32_t* d_seg_off, int n_clusters,
                      const double* d_plane4, int min_points, int max_points, double max_min_height, double min_max_height,
                      double min_height, double max_height, float* d_stats6, uint8_t* d_valid, void* stream) {
    if (n_clusters <= 0) return VG_OK;
    if (!d_points || !d_index || !d_seg_off || !d_plane4 || !d_stats6 || !d_valid) return VG_ERR_ARG;
    hipLaunchKernelGGL(k_cluster_filter, dim3(n_clusters), dim3(256), 0, (hipStream_t)stream, d_points, stride, d_index, d_seg_off,
                       d_plane4, min_points, max_points, max_min_height, min_max_height, min_height, max_height, d_stats6, d_valid);
    VG_LAUNCH_CHECK();
    return VG_OK;
}

void vg_filter_default_params(vg_filter_params* p) {
    memset(p, 0, sizeof(*p));
    p->min_points = 0;                       // cluster_utils.py:14
    p->max_points = 999999;
    p->min_height = -1e300; p->max_height = 1e300;
    p->min_aspect_ratio = -1e300; p->max_aspect_ratio = 1e300;
    p->min_volume = -1e300; p->max_volume = 1e300;
    p->min_area = -1e300; p->max_area = 1e300;
    p->max_min_height = 1e300; p->min_max_height = -1e300;
    p->percentile = 50.0; p->min_percentile_pp_score = 1e300;
}

int vg_cluster_filter_ex(const float* d_points, int stride, const int32_t* d_index, const int32_t* d_seg_off, int n_clusters,
                         const double* d_plane4, const float* d_scores, const vg_filter_params* p, double* d_stats,
                         uint8_t* d_verdict, uint8_t* d_valid, void* stream) {
    if (n_clusters <= 0) return VG_OK;
    if (!d_points || !d_index || !d_seg_off || !d_plane4 || !p || !d_stats || !d_verdict || !d_valid || stride < 3) return VG_ERR_ARG;
    for (int k = 0; k < VG_FILTER_COUNT; ++k)
        if (p->active[k] && (p->logic[k] < VG_FILTER_AND_REQUIRED || p->logic[k] > VG_FILTER_OR)) return VG_ERR_ARG;
    if (p->active[VG_FILTER_EPHEMERAL_SCORE] && (!d_scores || !(p->percentile >= 0.0 && p->percentile <= 100.0))) return VG_ERR_ARG;
    const int grid = n_clusters < 2048 ? n_clusters : 2048;          // 256 CUs x 8 resident workgroups: larger lists walk the grid
    hipLaunchKernelGGL(k_cluster_filter_ex, dim3(grid), dim3(256), 0, (hipStream_t)stream, d_points, stride, d_index, d_seg_off,
                       n_clusters, d_plane4, d_scores, *p, d_stats, d_verdict, d_valid);
    VG_LAUNCH_CHECK();
    return VG_OK;
}

int vg_cluster_boxes(const float* d_points, int stride, const int32_t* d_index, const int32_t* d_seg_off, int n_clusters,
                     double* d_box7, float* d_aux3, void* stream) {
    if (n_clusters <= 0) return VG_OK;
    if (!d_points || !d_index || !d_seg_off || !d_box7 || !d_aux3) return VG_ERR_ARG;
    hipLaunchKernelGGL(k_cluster_box, dim3(n_clusters), dim3(256), 0, (hipStream_t)stream, d_points, stride, d_index, d_seg_off,
                       d_box7, d_aux3);
    VG_LAUNCH_CHECK();
    return VG_OK;
}

int vg_entropy_scores(const int32_t* d_counts, int n_frames, int nq, int seek_row, double* d_H, void* stream) {
    if (nq < 0 || n_frames < 2 || n_frames > 128) return VG_ERR_ARG;
    if (nq == 0) return VG_OK;
    if (!d_counts || !d_H) return VG_ERR_ARG;
    hipLaunchKernelGGL(k_entropy_scores, dim3(vg_div_up(nq, 128)), dim3(128), 0, (hipStream_t)stream, d_counts, n_frames, nq,
                       seek_row, d_H);
    VG_LAUNCH_CHECK();
    return VG_OK;
}

int vg_subsample_keys(uint64_t seed, uint64_t tag, int n, int64_t* d_keys, void* stream) {
    if (n < 0) return VG_ERR_ARG;
    if (n == 0) return VG_OK;
    if (!d_keys) return VG_ERR_ARG;
    hipLaunchKernelGGL(k_subsample_keys, dim3(vg_div_up(n, 256)), dim3(256), 0, (hipStream_t)stream, seed, tag, n,
                       (long long*)d_keys);
    VG_LAUNCH_CHECK();
    return VG_OK;
}

}  // extern "C"
