// DBSCAN on the handle's cell grid: vg_cluster_dbscan / vg_dbscan_host (included by cluster.hip, which owns the grid, its sorted point
// copy, cl_box_d2, the rocprim scratch this file uses, and the working arrays it borrows: ClDbscanView).
//
// sklearn.cluster.DBSCAN, the second model the reference's cluster_utils.py imports (src/utils/cluster_utils.py:4-5), as the rules
// its `dbscan_inner` computes, stated without its traversal (include/vilgod_hip.h has the contract):
//   pair     dbscan_pair (dbscan_pair.inc): float64 d2 <= eps2, inclusive; a row is its own neighbour
//   core     a row with at least min_samples neighbours
//   cluster  a connected component of the neighbour graph on the core rows; numbered 0, 1, ... by its lowest core row
//   border   a non-core row takes the smallest label among its core neighbours, -1 when it has none
// Stages, one lane per row in sorted (Morton) order, every grid sized from n, nothing read back:
//   k_db_core     count neighbours in the cells around the row, stop at min_samples               -> core flag
//   k_db_union    union-find over sorted positions: a core row unites with core neighbours at LOWER positions
//   k_db_roots    every core row finds its root (read only) and offers its original row to the root's minimum (atomicMin)
//   k_db_mark     the row that IS its component's minimum raises its flag, in original order
//   rocprim exclusive scan of the n flags: a component's label, and the total
//   k_db_label    core rows read their root's label
//   k_db_border   non-core rows walk their cells again for the smallest label among core neighbours; every row then writes
//                 its results through perm into the caller's order (the scatter needs nothing the border pass does not hold)
// Integer atomics only, and only where the result is a set property (which rows are connected) or a minimum: the outputs are
// the same bits on every run.
//
// The cells of a walk.  A neighbour is at most eps away along every axis, so it sits at most ceil(eps / cell) cells away -- by the
// real faces.  The computed faces (cl_face) are off by ~1e-13 m, which matters only when eps is a whole number of cells: the walk
// therefore spans ceil(eps / cell + 1e-6) cells, one more shell than ceil(eps / cell) in exactly that case.  What is skipped inside
// the span is decided by cl_box_d2 alone, a proven lower bound of the float64 pair distance over x, y, z (tests/test_mst_edges.py);
// a 4th and 5th coordinate only add to d2.  cl_box_d2 = (gx^2 + gy^2) + gz^2 >= each of its terms (rounding is monotone), so a
// whole slab or row of cells whose own gap already exceeds eps2 is skipped before its cells are formed.

#define DB_NT 256

template <int DIM>
__device__ __forceinline__ DbRow db_row(const float4* __restrict__ spts, const float* __restrict__ st, int j) {
    const float4 p = spts[j];
    DbRow r;
    r.x = p.x; r.y = p.y; r.z = p.z; r.e = p.w;
    r.t = DIM >= 5 ? st[j] : 0.f;
    return r;
}

// visit(j0, j1) for every cell within `span` cells of q's own whose box can hold a neighbour; visit returns true to end the walk
template <typename Visit>
__device__ __forceinline__ void db_walk(const ClGrid& g, const DbRow& q, const int* __restrict__ cs, int span, double eps2, Visit&& visit) {
    const double qx = q.x, qy = q.y, qz = q.z;
    int cx, cy, cz;
    cl_cell_of(g, qx, qy, qz, cx, cy, cz);
    for (int z = max(cz - span, 0); z <= min(cz + span, CL_NZ - 1); ++z) {
        const double gz = cl_axis_gap(g.oz, qz, z, 0, CL_NZ);
        if (gz * gz > eps2) continue;
        for (int y = max(cy - span, 0); y <= min(cy + span, CL_NY - 1); ++y) {
            const double gy = cl_axis_gap(g.oy, qy, y, 0, CL_NY);
            if (gy * gy > eps2) continue;
            for (int x = max(cx - span, 0); x <= min(cx + span, CL_NX - 1); ++x) {
                if (cl_box_d2(g, qx, qy, qz, 0, x, y, z) > eps2) continue;      // strictly: a box AT eps2 can hold a neighbour
                const unsigned int c = cl_code(x, y, z);
                const int j0 = cl_start(cs, c), j1 = cl_start(cs, c + 1u);
                if (j0 < j1 && visit(j0, j1)) return;
            }
        }
    }
}

template <int DIM>
__global__ __launch_bounds__(DB_NT) void k_db_core(const float4* __restrict__ spts, const float* __restrict__ st, int n,
                                                   const ClGrid* __restrict__ gp, const int* __restrict__ cs,
                                                   const int* __restrict__ perm, int span, double eps2, int min_samples,
                                                   int* __restrict__ core, int* __restrict__ parent, int* __restrict__ minrow,
                                                   int* __restrict__ flag, int* __restrict__ status) {
    const int i = blockIdx.x * DB_NT + threadIdx.x;
    if (i == 0) *status = 0;                          // (the later launches raise it; this one never reads it)
    if (i >= n) return;
    const ClGrid g = *gp;
    const DbRow q = db_row<DIM>(spts, st, i);
    int cnt = 0;
    db_walk(g, q, cs, span, eps2, [&](int j0, int j1) {
        for (int j = j0; j < j1 && cnt < min_samples; ++j) cnt += dbscan_pair(DIM, q, db_row<DIM>(spts, st, j), eps2) ? 1 : 0;
        return cnt >= min_samples;
    });
    core[i] = cnt >= min_samples ? 1 : 0;
    parent[i] = i;
    minrow[i] = 0x7FFFFFFF;
    flag[perm[i]] = 0;
}

// ---- union-find over sorted positions ------------------------------------------------------------------------------------
// INVARIANT: parent[p] <= p at all times, and parent[p] is a member of p's component.  A root (parent[r] == r) is only ever
// re-pointed to a SMALLER root, by atomicCAS(&parent[hi], hi, lo); a non-root is only ever re-pointed to a smaller ancestor
// (atomicMin, path halving).  So every find walk strictly descends and ends within p steps, the smallest position of a component
// is never re-pointed and ends as its root, and the components are those of the edge set whatever order the hardware runs the
// unions in.  Every read of parent[] during the launch is an agent-scope atomic load: a plain load may be served from this CU's
// L1 and miss another workgroup's update (a stale value is still an ancestor, so it would cost steps, not correctness).
// Every walk and every retry loop is bounded by n all the same; an overrun raises the status word and gives up: no spinning.
__device__ __forceinline__ int db_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

template <bool HALVE>
__device__ __forceinline__ int db_find(int* parent, int p, int n, int* status) {
    for (int steps = 0; steps <= n; ++steps) {
        const int q = db_load(parent + p);
        if (q == p) return p;
        if (HALVE) {
            const int gq = db_load(parent + q);
            if (gq < q) atomicMin(parent + p, gq);
        }
        p = q;
    }
    atomicOr(status, 1);
    return p;
}

__device__ __forceinline__ void db_unite(int* parent, int a, int b, int n, int* status) {
    for (int tries = 0; tries <= n; ++tries) {
        a = db_find<true>(parent, a, n, status);
        b = db_find<true>(parent, b, n, status);
        if (a == b) return;
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        const int old = atomicCAS(parent + hi, hi, lo);
        if (old == hi) return;
        a = old;                                      // hi had been hooked meanwhile: go on from where it points (old < hi)
        b = lo;
    }
    atomicOr(status, 2);
}

template <int DIM>
__global__ __launch_bounds__(DB_NT) void k_db_union(const float4* __restrict__ spts, const float* __restrict__ st, int n,
                                                    const ClGrid* __restrict__ gp, const int* __restrict__ cs, int span, double eps2,
                                                    const int* __restrict__ core, int* parent, int* status) {
    const int i = blockIdx.x * DB_NT + threadIdx.x;
    if (i >= n || !core[i]) return;
    const ClGrid g = *gp;
    const DbRow q = db_row<DIM>(spts, st, i);
    db_walk(g, q, cs, span, eps2, [&](int j0, int j1) {
        const int je = j1 < i ? j1 : i;               // lower sorted positions only: every edge is united once
        for (int j = j0; j < je; ++j)
            if (core[j] && dbscan_pair(DIM, q, db_row<DIM>(spts, st, j), eps2)) db_unite(parent, i, j, n, status);
        return false;
    });
}

__global__ __launch_bounds__(DB_NT) void k_db_roots(int n, const int* __restrict__ core, const int* __restrict__ perm, int* parent,
                                                    int* __restrict__ root, int* __restrict__ minrow, int* status) {
    const int i = blockIdx.x * DB_NT + threadIdx.x;
    if (i >= n) return;
    int r = -1;
    if (core[i]) {
        r = db_find<false>(parent, i, n, status);     // the unions are over: parent[] is read only here
        atomicMin(minrow + r, perm[i]);
    }
    root[i] = r;
}

__global__ __launch_bounds__(DB_NT) void k_db_mark(int n, const int* __restrict__ root, const int* __restrict__ perm,
                                                   const int* __restrict__ minrow, int* __restrict__ flag) {
    const int i = blockIdx.x * DB_NT + threadIdx.x;
    if (i >= n) return;
    const int r = root[i];
    if (r >= 0 && minrow[r] == perm[i]) flag[perm[i]] = 1;
}

__global__ __launch_bounds__(DB_NT) void k_db_label(int n, const int* __restrict__ root, const int* __restrict__ minrow,
                                                    const int* __restrict__ flag, const int* __restrict__ scan,
                                                    const int* __restrict__ status, int* __restrict__ label_s,
                                                    int* __restrict__ n_clusters) {
    const int i = blockIdx.x * DB_NT + threadIdx.x;
    if (i >= n) return;
    const int r = root[i];
    const int m = r >= 0 ? minrow[r] : -1;            // a root's minimum is a row; after an overrun `r` may be no root: then no label
    label_s[i] = m >= 0 && m < n ? scan[m] : -1;
    if (i == n - 1) *n_clusters = *status ? -1 : scan[n - 1] + flag[n - 1];
}

template <int DIM>
__global__ __launch_bounds__(DB_NT) void k_db_border(const float4* __restrict__ spts, const float* __restrict__ st, int n,
                                                     const ClGrid* __restrict__ gp, const int* __restrict__ cs,
                                                     const int* __restrict__ perm, int span, double eps2,
                                                     const int* __restrict__ core, const int* __restrict__ label_s,
                                                     int* __restrict__ labels, unsigned char* __restrict__ core_out,
                                                     double* __restrict__ probs) {
    const int i = blockIdx.x * DB_NT + threadIdx.x;
    if (i >= n) return;
    const int is_core = core[i];
    int lab = label_s[i];
    if (!is_core) {
        const ClGrid g = *gp;
        const DbRow q = db_row<DIM>(spts, st, i);
        int best = 0x7FFFFFFF;
        db_walk(g, q, cs, span, eps2, [&](int j0, int j1) {
            for (int j = j0; j < j1; ++j) {
                if (!core[j]) continue;
                const int lj = label_s[j];
                if (lj < best && dbscan_pair(DIM, q, db_row<DIM>(spts, st, j), eps2)) best = lj;
            }
            return best == 0;                         // no label is smaller
        });
        lab = best == 0x7FFFFFFF ? -1 : best;
    }
    const int o = perm[i];
    labels[o] = lab;
    core_out[o] = (unsigned char)is_core;
    if (probs) probs[o] = lab >= 0 ? 1.0 : 0.0;
}

// the walk's span in cells and eps2, or false for an eps the grid cannot serve (NaN, <= 0, ceil(eps / cell) > 8)
static bool db_eps(double eps, int* span, double* eps2) {
    if (!(eps > 0.0) || ceil(eps / CL_CELL) > 8.0) return false;
    *span = (int)ceil(eps / CL_CELL + 1e-6);
    *eps2 = eps * eps;
    return true;
}

template <int DIM>
static int db_run(vg_cluster* h, const float* d_points, int n, int stride, int span, double eps2, int min_samples, int32_t* d_labels,
                  uint8_t* d_core, double* d_probs, int32_t* d_n_clusters, hipStream_t st) {
    {
        const int rc = cl_build_grid(h, d_points, n, stride, DIM, st, true);
        if (rc != VG_OK) return rc;
    }
    const ClDbscanView v = cl_dbscan_view(h);         // the working arrays, [max_points] each
    const dim3 grid(vg_div_up(n, DB_NT)), block(DB_NT);
    hipLaunchKernelGGL((k_db_core<DIM>), grid, block, 0, st, h->d_spts, h->d_st, n, h->d_grid, h->d_cell_start, h->d_perm, span, eps2,
                       min_samples, v.core, v.parent, v.minrow, v.flag, v.status);
    hipLaunchKernelGGL((k_db_union<DIM>), grid, block, 0, st, h->d_spts, h->d_st, n, h->d_grid, h->d_cell_start, span, eps2, v.core, v.parent,
                       v.status);
    hipLaunchKernelGGL(k_db_roots, grid, block, 0, st, n, v.core, h->d_perm, v.parent, v.root, v.minrow, v.status);
    hipLaunchKernelGGL(k_db_mark, grid, block, 0, st, n, v.root, h->d_perm, v.minrow, v.flag);
    size_t tb = h->temp_bytes;
    VG_CHECK(rocprim::exclusive_scan(h->d_temp, tb, v.flag, v.scan, 0, (size_t)n, rocprim::plus<int>(), st));
    hipLaunchKernelGGL(k_db_label, grid, block, 0, st, n, v.root, v.minrow, v.flag, v.scan, v.status, v.label_s, d_n_clusters);
    hipLaunchKernelGGL((k_db_border<DIM>), grid, block, 0, st, h->d_spts, h->d_st, n, h->d_grid, h->d_cell_start, h->d_perm, span, eps2,
                       v.core, v.label_s, d_labels, d_core, d_probs);
    VG_LAUNCH_CHECK();
    return VG_OK;
}

extern "C" {

int vg_cluster_dbscan(vg_cluster* h, const float* d_points, int n, int stride, int dim, double eps, int min_samples, int32_t* d_labels,
                      uint8_t* d_core, double* d_probs, int32_t* d_n_clusters, void* stream) {
    int span;
    double eps2;
    if (!h || n < 0 || dim < 3 || dim > 5 || stride < dim || min_samples < 1 || !db_eps(eps, &span, &eps2) || !d_n_clusters)
        return VG_ERR_ARG;
    if (n > h->max_points) return VG_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    h->grid_n = 0;
    if (n == 0) {
        VG_CHECK(hipMemsetAsync(d_n_clusters, 0, 4, st));
        return VG_OK;
    }
    if (!d_points || !d_labels || !d_core) return VG_ERR_ARG;
    return cl_with_dim(dim, [&](auto d) {
        return db_run<decltype(d)::value>(h, d_points, n, stride, span, eps2, min_samples, d_labels, d_core, d_probs, d_n_clusters, st);
    });
}

// HOST ONLY: all pairs, no grid, a sequential union-find, the same pair function
int vg_dbscan_host(const float* h_points, int n, int stride, int dim, double eps, int min_samples, int32_t* h_labels, uint8_t* h_core,
                   double* h_probs, int32_t* h_n_clusters) {
    int span;
    double eps2;
    if (n < 0 || dim < 3 || dim > 5 || stride < dim || min_samples < 1 || !db_eps(eps, &span, &eps2) || !h_n_clusters) return VG_ERR_ARG;
    *h_n_clusters = 0;
    if (n == 0) return VG_OK;
    if (!h_points || !h_labels || !h_core) return VG_ERR_ARG;
    auto row = [&](int i) {
        const float* p = h_points + (size_t)i * stride;
        DbRow r;
        r.x = p[0]; r.y = p[1]; r.z = p[2];
        r.e = dim >= 4 ? p[3] : 0.f;
        r.t = dim >= 5 ? p[4] : 0.f;
        return r;
    };
    std::vector<DbRow> rows(n);
    for (int i = 0; i < n; ++i) rows[i] = row(i);
    std::vector<int> cnt(n, 1);                       // a row is its own neighbour
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < i; ++j)
            if (dbscan_pair(dim, rows[i], rows[j], eps2)) { ++cnt[i]; ++cnt[j]; }
    for (int i = 0; i < n; ++i) h_core[i] = cnt[i] >= min_samples ? 1 : 0;
    std::vector<int> parent(n);
    for (int i = 0; i < n; ++i) parent[i] = i;
    auto find = [&](int p) {
        int r = p;
        while (parent[r] != r) r = parent[r];
        while (parent[p] != r) { const int q = parent[p]; parent[p] = r; p = q; }
        return r;
    };
    for (int i = 0; i < n; ++i) {
        if (!h_core[i]) continue;
        for (int j = 0; j < i; ++j) {
            if (!h_core[j] || !dbscan_pair(dim, rows[i], rows[j], eps2)) continue;
            const int a = find(i), b = find(j);
            if (a != b) parent[a > b ? a : b] = a > b ? b : a;      // the root is the component's lowest row
        }
    }
    // rows ascending: a core row that is its own root is its component's lowest core row
    int nc = 0;
    for (int i = 0; i < n; ++i) h_labels[i] = -1;
    for (int i = 0; i < n; ++i)
        if (h_core[i]) {
            const int r = find(i);
            if (r == i) h_labels[i] = nc++;
            else h_labels[i] = h_labels[r];
        }
    for (int i = 0; i < n; ++i) {
        if (h_core[i]) continue;
        int best = -1;
        for (int j = 0; j < n; ++j)
            if (h_core[j] && (best < 0 || h_labels[j] < best) && dbscan_pair(dim, rows[i], rows[j], eps2)) best = h_labels[j];
        h_labels[i] = best;
    }
    if (h_probs)
        for (int i = 0; i < n; ++i) h_probs[i] = h_labels[i] >= 0 ? 1.0 : 0.0;
    *h_n_clusters = nc;
    return VG_OK;
}

}  // extern "C"
