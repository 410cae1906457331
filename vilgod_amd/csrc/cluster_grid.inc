// Part of cluster.hip (included in place): K2a, the grid build -- bounding box, origin, Morton codes, the sort, the sorted point copy, the
// cell-start table with its coarser levels (cl_build_grid), and the per-node range of the 4th clustering coordinate (k_cl_e_*).
// Expects cluster_geom.inc, vg_cluster and rocprim.

__global__ void k_cl_levels(int* __restrict__ cs) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= CL_LVL_TOTAL) return;
    int l = 1;
    while (l < CL_LMAX && idx >= cl_lvl_off(l + 1)) ++l;
    const size_t c = idx - cl_lvl_off(l);
    cs[(size_t)(CL_NCODES + 1) + idx] = cs[(size_t)CL_NCODES - (c << (3 * l))];
}

__global__ void k_cl_bbox(const float* __restrict__ pts, int n, int stride, ClGrid* g) {
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            float v = pts[(size_t)i * stride + a];
            mn[a] = fminf(mn[a], v);
            mx[a] = fmaxf(mx[a], v);
        }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        mn[a] = vg_wave_min(mn[a]);
        mx[a] = vg_wave_max(mx[a]);
    }
    // one set of atomics per BLOCK (64 blocks): 7.4 k atomics of 1 236 waves on the same cache line took 87 us
    __shared__ float red[4][6];
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int a = 0; a < 3; ++a) { red[threadIdx.x >> 6][a] = mn[a]; red[threadIdx.x >> 6][3 + a] = mx[a]; }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int a = threadIdx.x;
        float lo = red[0][a], hi = red[0][3 + a];
        for (int w = 1; w < (int)(blockDim.x >> 6); ++w) { lo = fminf(lo, red[w][a]); hi = fmaxf(hi, red[w][3 + a]); }
        atomicMin(&g->kmin[a], vg_fkey(lo));
        atomicMax(&g->kmax[a], vg_fkey(hi));
    }
}

// the ClGrid a build starts from, written on the device: what cl_build_grid otherwise copies from the host, for calls that are captured
// into a graph (a copy node would read the host bytes again at every replay)
__global__ void k_cl_grid_reset(ClGrid* g) {
    if (threadIdx.x != 0) return;
    g->ox = 0.0; g->oy = 0.0; g->oz = 0.0;
    for (int a = 0; a < 3; ++a) { g->kmin[a] = 0xFFFFFFFFu; g->kmax[a] = 0u; }
    g->inf = __hiloint2double(0x7FF00000, 0);
}

__global__ void k_cl_grid(ClGrid* g) {
    if (threadIdx.x != 0) return;
    double lo[3], hi[3];
    for (int a = 0; a < 3; ++a) {
        lo[a] = vg_fkey_inv(g->kmin[a]);
        hi[a] = vg_fkey_inv(g->kmax[a]);
    }
    const double ext[3] = {CL_NX * CL_CELL, CL_NY * CL_CELL, CL_NZ * CL_CELL};
    double o[3];
    for (int a = 0; a < 3; ++a) o[a] = cl_origin(lo[a], hi[a], ext[a]);
    g->ox = o[0]; g->oy = o[1]; g->oz = o[2];
}

__global__ void k_cl_codes(const float* __restrict__ pts, int n, int stride, const ClGrid* __restrict__ g,
                           unsigned int* __restrict__ code, int* __restrict__ perm) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int cx, cy, cz;
    cl_cell_of(*g, pts[(size_t)i * stride], pts[(size_t)i * stride + 1], pts[(size_t)i * stride + 2], cx, cy, cz);
    code[i] = cl_code(cx, cy, cz);
    perm[i] = i;
}

__global__ void k_cl_gather(const float* __restrict__ pts, int n, int stride, int dim, const int* __restrict__ perm,
                            const unsigned int* __restrict__ code_s, float4* __restrict__ spts, float* __restrict__ st,
                            int* __restrict__ cell_start_rev) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* p = pts + (size_t)perm[i] * stride;
    spts[i] = make_float4(p[0], p[1], p[2], dim >= 4 ? p[3] : 0.f);
    if (dim >= 5) st[i] = p[4];
    if (i == 0 || code_s[i] != code_s[i - 1]) cell_start_rev[CL_NCODES - code_s[i]] = i;
}

__global__ void k_cl_fill_int(int* p, int v, size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

// ---- range of the 4th clustering coordinate per octree node (levels 0..CL_PUR_LEVELS-1), for the 4-/5-D searches -----
// The grid prunes on x,y,z only; in the two-frame input the 4th coordinate (entropy score, 0..1) often separates a
// point from ALL its spatial neighbours, so the xyz bound alone lets the search wander through thousands of points that
// are close in space and far in 5-D.  Packed as two fp16: min rounded DOWN (low half), max rounded UP (high half).
__device__ __forceinline__ unsigned int cl_pack_e(float mn, float mx) {
    __half hmn = __float2half_rd(mn), hmx = __float2half_ru(mx);
    return (unsigned int)__half_as_ushort(hmn) | ((unsigned int)__half_as_ushort(hmx) << 16);
}
__device__ __forceinline__ void cl_unpack_e(unsigned int v, float& mn, float& mx) {
    mn = __half2float(__ushort_as_half((unsigned short)(v & 0xFFFFu)));
    mx = __half2float(__ushort_as_half((unsigned short)(v >> 16)));
}
// squared gap between qe and the node's [min, max] range (0 inside), shaved by 2^-30 so that rounding cannot lift the
// sum above the true minimum
__device__ __forceinline__ double cl_e_gap2(unsigned int packed, double qe) {
    float mn, mx;
    cl_unpack_e(packed, mn, mx);
    double d = 0.0;
    if (qe < (double)mn) d = (double)mn - qe;
    else if (qe > (double)mx) d = qe - (double)mx;
    d *= (1.0 - 9.313225746154785e-10);
    return d * d;
}
__global__ void k_cl_e_leaf(int n, const unsigned int* __restrict__ code_s, const float4* __restrict__ spts,
                            unsigned int* __restrict__ cell_e) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned int c = code_s[i];
    if (i > 0 && code_s[i - 1] == c) return;
    float mn = spts[i].w, mx = mn;
    for (int j = i + 1; j < n && code_s[j] == c; ++j) {
        const float e = spts[j].w;
        mn = fminf(mn, e);
        mx = fmaxf(mx, e);
    }
    cell_e[c] = cl_pack_e(mn, mx);
}
__global__ void k_cl_e_up(int n, int l, const unsigned int* __restrict__ code_s, const int* __restrict__ cs,
                          unsigned int* __restrict__ cell_e) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned int key = code_s[i] >> (3 * l);
    if (i > 0 && (code_s[i - 1] >> (3 * l)) == key) return;
    const unsigned int* below = cell_e + cl_pur_off_fwd(l - 1);
    float mn = INFINITY, mx = -INFINITY;
    for (unsigned int ch = 0; ch < 8; ++ch) {
        const unsigned int ck = key * 8 + ch;
        const unsigned int c0 = ck << (3 * (l - 1));
        if (cl_start_l(cs, l - 1, c0 >> (3 * (l - 1))) == cl_start_l(cs, l - 1, (c0 >> (3 * (l - 1))) + 1u)) continue;   // empty child: entry not written
        float a, b;
        cl_unpack_e(below[ck], a, b);
        mn = fminf(mn, a);
        mx = fmaxf(mx, b);
    }
    cell_e[cl_pur_off_fwd(l) + key] = cl_pack_e(mn, mx);
}

// ---------------------------------------------------------------------------------------------
struct MinOp {
    __device__ __host__ int operator()(int a, int b) const { return a < b ? a : b; }
};

// bbox -> grid origin -> Morton codes -> radix sort -> sorted points + dense cell-start table
// (device_reset: the starting ClGrid is written by a kernel instead of copied from the host -- vg_cluster_dbscan, which can be captured)
static int cl_build_grid(vg_cluster* h, const float* d_points, int n, int stride, int dim, hipStream_t st, bool device_reset = false) {
    const int nb = vg_div_up(n, 256);
    if (device_reset) {
        hipLaunchKernelGGL(k_cl_grid_reset, dim3(1), dim3(64), 0, st, h->d_grid);
    } else {
        ClGrid g0;
        memset(&g0, 0, sizeof(g0));
        for (int a = 0; a < 3; ++a) { g0.kmin[a] = 0xFFFFFFFFu; g0.kmax[a] = 0u; }
        g0.inf = INFINITY;
        VG_CHECK(hipMemcpyAsync(h->d_grid, &g0, sizeof(g0), hipMemcpyHostToDevice, st));
    }
    hipLaunchKernelGGL(k_cl_bbox, dim3(std::min(nb, 64)), dim3(256), 0, st, d_points, n, stride, h->d_grid);
    hipLaunchKernelGGL(k_cl_grid, dim3(1), dim3(64), 0, st, h->d_grid);
    hipLaunchKernelGGL(k_cl_codes, dim3(nb), dim3(256), 0, st, d_points, n, stride, h->d_grid, h->d_code, h->d_perm_in);
    size_t tb = h->temp_bytes;
    VG_CHECK(rocprim::radix_sort_pairs(h->d_temp, tb, h->d_code, h->d_code_s, h->d_perm_in, h->d_perm, (size_t)n, 0, 24, st));
    {
        size_t tot = (size_t)CL_NCODES + 1;
        hipLaunchKernelGGL(k_cl_fill_int, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, h->d_cell_start, n, tot);
    }
    hipLaunchKernelGGL(k_cl_gather, dim3(nb), dim3(256), 0, st, d_points, n, stride, dim, h->d_perm, h->d_code_s, h->d_spts,
                       h->d_st, h->d_cell_start);
    tb = h->temp_bytes;
    VG_CHECK(rocprim::inclusive_scan(h->d_temp, tb, h->d_cell_start, h->d_cell_start, (size_t)(CL_NCODES + 1), MinOp(), st));
    hipLaunchKernelGGL(k_cl_levels, dim3((unsigned)((CL_LVL_TOTAL + 255) / 256)), dim3(256), 0, st, h->d_cell_start);
    VG_LAUNCH_CHECK();
    h->grid_n = n;
    return VG_OK;
}
