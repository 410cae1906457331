// Part of cluster.hip (included in place): the fixed-radius queries on the grid of a TARGET set -- k_cl_ball_count, k_cl_nearest and
// their entry points vg_cluster_ball_count / vg_cluster_nearest.  cluster_knn.inc, the K nearest targets without a radius, comes behind
// it and shares cl_d2_f32.  Expects cluster_geom.inc and vg_cluster (the grid buffers and grid_n).

// ---------------------------------------------------------------------------------------------
// Fixed-radius queries against the grid of a TARGET point set (entropy scores / two-frame clustering, SURVEY 8f N1).
// float32 arithmetic in the order the reference's CUDA ops compile to under nvcc's default FMA contraction:
//   d2 = fma(dz, dz, fma(dy, dy, dx * dx))      (pcdet ball_query_kernel_stack; pytorch3d KNearestNeighbor dist += diff*diff)
__host__ __device__ __forceinline__ float cl_d2_f32(float qx, float qy, float qz, const float4& b) {
    const float dx = qx - b.x, dy = qy - b.y, dz = qz - b.z;
    return fmaf(dz, dz, fmaf(dy, dy, dx * dx));
}

// counts[i] = min(cap, #{ target j : d2(q_i, t_j) < r2 })  -- pointcloud_utils.py:74-107 (ball_query + count_nonzero)
// squared distance (float, slightly UNDER-estimated) from q to cell (x,y,z) of the grid: a cell is skipped only when even
// this lower bound exceeds the radius.  Border cells extend to infinity outwards (points beyond the grid are clamped into them).
__device__ __forceinline__ float cl_cell_d2_lb(const ClGrid& g, float qx, float qy, float qz, int x, int y, int z) {
    const float q[3] = {qx, qy, qz};
    const double o[3] = {g.ox, g.oy, g.oz};
    const int c[3] = {x, y, z}, nb[3] = {CL_NX, CL_NY, CL_NZ};
    float d2 = 0.f;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float lo = (float)cl_face(o[a], c[a], 0), hi = (float)cl_face(o[a], c[a] + 1, 0);
        float d = 0.f;
        if (q[a] < lo && c[a] > 0) d = lo - q[a];
        else if (q[a] > hi && c[a] < nb[a] - 1) d = q[a] - hi;
        d2 += d * d;
    }
    return d2 * 0.9999f - 1e-6f;
}

__global__ __launch_bounds__(256) void k_cl_ball_count(const float* __restrict__ q, int nq, int qstride,
                                                       const float4* __restrict__ spts, const ClGrid* __restrict__ gp,
                                                       const int* __restrict__ cs, float r2, int reach, int cap,
                                                       int* __restrict__ counts) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    const ClGrid g = *gp;
    const float qx = q[(size_t)i * qstride], qy = q[(size_t)i * qstride + 1], qz = q[(size_t)i * qstride + 2];
    int cx, cy, cz;
    cl_cell_of(g, qx, qy, qz, cx, cy, cz);
    int cnt = 0;
    for (int z = max(cz - reach, 0); z <= min(cz + reach, CL_NZ - 1); ++z)
        for (int y = max(cy - reach, 0); y <= min(cy + reach, CL_NY - 1); ++y)
            for (int x = max(cx - reach, 0); x <= min(cx + reach, CL_NX - 1); ++x) {
                if (cl_cell_d2_lb(g, qx, qy, qz, x, y, z) >= r2) continue;          // no point of this cell can be inside
                const unsigned int c = cl_code(x, y, z);
                const int j0 = cl_start(cs, c), j1 = cl_start(cs, c + 1u);
                for (int j = j0; j < j1; ++j) cnt += cl_d2_f32(qx, qy, qz, spts[j]) < r2 ? 1 : 0;
                if (cnt >= cap) { counts[i] = cap; return; }                        // the reference stops at nsample hits
            }
    counts[i] = cnt < cap ? cnt : cap;
}

// nearest target point with d2 <= r2max: idx (ORIGINAL target index, lowest index among equidistant ones) and d2, or
// (-1, +inf)  -- pointcloud_utils.py:496-513 (knn K=1 + distance gate)
__global__ __launch_bounds__(256) void k_cl_nearest(const float* __restrict__ q, int nq, int qstride,
                                                    const float4* __restrict__ spts, const int* __restrict__ perm,
                                                    const ClGrid* __restrict__ gp, const int* __restrict__ cs, float r2max,
                                                    int reach, int* __restrict__ idx, float* __restrict__ d2out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    const ClGrid g = *gp;
    const float qx = q[(size_t)i * qstride], qy = q[(size_t)i * qstride + 1], qz = q[(size_t)i * qstride + 2];
    int cx, cy, cz;
    cl_cell_of(g, qx, qy, qz, cx, cy, cz);
    float best = INFINITY;
    int bi = -1;
    auto scan = [&](int x, int y, int z) {
        const unsigned int c = cl_code(x, y, z);
        const int j0 = cl_start(cs, c), j1 = cl_start(cs, c + 1u);
        for (int j = j0; j < j1; ++j) {
            const float d2 = cl_d2_f32(qx, qy, qz, spts[j]);
            if (d2 > r2max) continue;
            const int o = perm[j];
            if (d2 < best || (d2 == best && o < bi)) { best = d2; bi = o; }
        }
    };
    if (reach >= 0) scan(cx, cy, cz);                 // the own cell first: its hit prunes most of the others
    for (int z = max(cz - reach, 0); z <= min(cz + reach, CL_NZ - 1); ++z)
        for (int y = max(cy - reach, 0); y <= min(cy + reach, CL_NY - 1); ++y)
            for (int x = max(cx - reach, 0); x <= min(cx + reach, CL_NX - 1); ++x) {
                if (x == cx && y == cy && z == cz) continue;
                const float lb = cl_cell_d2_lb(g, qx, qy, qz, x, y, z);
                if (lb > r2max || lb > best) continue;        // equal distances still compete on the index: strict >
                scan(x, y, z);
            }
    idx[i] = bi;
    d2out[i] = best;
}

extern "C" {

/* d_counts[i] = min(cap, number of grid points t with d2(q_i, t) < r2), float32 d2 = fma(dz,dz,fma(dy,dy,dx*dx))
 * (pcdet ball_query + the count of pointcloud_utils.py:74-107; a query point that is itself in the target set counts). */
int vg_cluster_ball_count(vg_cluster* h, const float* d_query, int nq, int qstride, float r2, int cap, int32_t* d_counts,
                          void* stream) {
    if (!h || nq < 0 || qstride < 3 || !(r2 > 0.f) || cap < 0) return VG_ERR_ARG;
    if (nq == 0) return VG_OK;
    if (!d_query || !d_counts) return VG_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (h->grid_n == 0) { VG_CHECK(hipMemsetAsync(d_counts, 0, 4 * (size_t)nq, st)); return VG_OK; }
    const int reach = (int)ceil(sqrt((double)r2) / CL_CELL);
    if (reach > 8) return VG_ERR_ARG;
    hipLaunchKernelGGL(k_cl_ball_count, dim3(vg_div_up(nq, 256)), dim3(256), 0, st, d_query, nq, qstride, h->d_spts, h->d_grid,
                       h->d_cell_start, r2, reach, cap, d_counts);
    VG_LAUNCH_CHECK();
    return VG_OK;
}

/* nearest grid point with float32 d2 <= max_d2: d_idx = its index in the point array given to vg_cluster_grid (lowest
 * index among equidistant points) and d_d2, or -1 / +inf (pointcloud_utils.py:496-513: knn K=1 + squared-distance gate). */
int vg_cluster_nearest(vg_cluster* h, const float* d_query, int nq, int qstride, float max_d2, int32_t* d_idx, float* d_d2,
                       void* stream) {
    if (!h || nq < 0 || qstride < 3 || !(max_d2 > 0.f)) return VG_ERR_ARG;
    if (nq == 0) return VG_OK;
    if (!d_query || !d_idx || !d_d2) return VG_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int reach = h->grid_n ? (int)ceil(sqrt((double)max_d2) / CL_CELL) : 0;
    if (reach > 8) return VG_ERR_ARG;
    hipLaunchKernelGGL(k_cl_nearest, dim3(vg_div_up(nq, 256)), dim3(256), 0, st, d_query, nq, qstride, h->d_spts, h->d_perm,
                       h->d_grid, h->d_cell_start, max_d2, h->grid_n ? reach : -1, d_idx, d_d2);
    VG_LAUNCH_CHECK();
    return VG_OK;
}

}  // extern "C"
