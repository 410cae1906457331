// K nearest targets without a radius limit: vg_cluster_knn / vg_knn_host (included by cluster.hip, which owns the grid, the implicit
// octree and the pair distance this file walks with).
//
// pytorch3d's `knn_points` as the reference calls it: pointcloud_utils.py:476-493 (chamfer_distance), :496-503 (knn), :505-513
// (knn_labels), zero_shot_detector.py:221 (K = 4 among the moving points) and :237 (the label transfer).  One lane per query walks the
// octree of the TARGET set depth-first, nearest child first, with the K best (d2, row) pairs so far instead of a radius:
//   * pair distance   cl_d2_f32, float32 fma(dz, dz, fma(dy, dy, dx * dx)): the function k_cl_nearest / k_cl_ball_count use
//   * order           STRICT and total: (d2, row in the array given to vg_cluster_grid) ascending, packed as ONE unsigned 64-bit key
//                     = float32 bits of d2 << 32 | row.  d2 is +0 .. +inf, never negative, never NaN (finite operands), so its bit
//                     pattern orders like its value.  The K smallest keys of a set do not depend on the order of arrival: the walk's
//                     order decides speed only.
//   * pruning         a node is skipped only when cl_knn_prune_bound(cl_box_d2) > the K-th best d2 so far (max_d2 until the list is
//                     full), strictly: a node that could hold an EQUAL d2 is opened, because equal distances compete on the row.
//
// The list.  K <= VG_KNN_K_REG8 lives in registers: KC = 1, 4 or 8 keys, ascending, entered by a min / max chain (ClRegList is the
// model).  A list with K < KC starts with KC - K keys of value 0 in front: no key is smaller, so they never move and the K real entries
// occupy the last K slots -- the worst entry is ALWAYS slot KC - 1 and no slot is ever addressed by a run-time index inside the walk.
// K > VG_KNN_K_REG8 lives in LDS: a per-lane MAX-heap of K keys, heap[r * NT + lane] (ClLdsHeap is the model: 64-bit entries,
// lane-interleaved, conflict-free under any divergence); the root is the worst entry; the output is a heap sort in place.
// Empty slots hold ~0: its high word is no float32 a distance can take and it sorts behind every key.

#define CL_KNN_EMPTY 0xFFFFFFFFFFFFFFFFull

// Lower bound of the FLOAT32 pair distance cl_d2_f32(q, t) over every target t of a node whose cl_box_d2(q, node) is `box_d2`.
//
// cl_box_d2 bounds the float64 pair distance D64 = fl64((ex*ex + ey*ey) + ez*ez), e = q - t formed in float64 (tests/test_mst_edges.py).
// With v = 2^-53: each e is the real difference E up to (1 + v) -- it is exact unless the operands are more than 2^29 apart in
// magnitude -- and the five float64 operations behind it each round by at most (1 + v), so  D64 <= R (1 + v)^7  with
// R = Ex^2 + Ey^2 + Ez^2 the REAL squared distance, i.e.  R >= box_d2 (1 - 7v).
// The float32 chain, u = 2^-24, a = the absolute error of one float32 operation whose result falls below 2^-126:
//   dx = fl32(qx - tx) = Ex (1 + d1), |d1| <= u.  No absolute term: a float32 sum or difference that is subnormal is exact.
//   p1 = fl32(dx * dx)      >= dx^2 (1 - u) - a
//   p2 = fl32(dy * dy + p1) >= (dy^2 + p1) (1 - u) - a          (one rounding: fmaf)
//   p3 = fl32(dz * dz + p2) >= (dz^2 + p2) (1 - u) - a
// and dx^2 >= Ex^2 (1 - u)^2, so the term with the longest chain gives  p3 >= R (1 - u)^5 - 3a >= R (1 - 5u) - 3a.
// a: with gradual underflow half a subnormal step, 2^-150; if the device flushed subnormal results (and inputs: a flushed difference is
// below 2^-126 and its square below 2^-252) at most 2^-126.  The bound takes the larger, so it holds in either mode: 3a = 3 * 2^-126.
// An overflowing chain gives +inf, above every bound.  Together:
//   cl_d2_f32 >= box_d2 (1 - 7v) (1 - 5u) - 3 * 2^-126 > box_d2 (1 - 6u) - 2^-124.
// The function evaluates  box_d2 * (1 - 2^-21) - 2^-124  in float64: 1 - 8u instead of 1 - 6u pays for its own two roundings (2v each)
// and leaves 2u of room; the price is a node opened in vain when it lies within 5e-7 (relative) of the K-th distance.
__host__ __device__ __forceinline__ double cl_knn_prune_bound(double box_d2) {
    return box_d2 * (1.0 - 4.76837158203125e-07) - 4.70197740328915e-38;      // 2^-21, 2^-124
}

__host__ __device__ __forceinline__ unsigned long long cl_knn_key(float d2, int row) {
#ifdef __HIP_DEVICE_COMPILE__
    const unsigned int b = __float_as_uint(d2);
#else
    unsigned int b;
    memcpy(&b, &d2, 4);
#endif
    return ((unsigned long long)b << 32) | (unsigned int)row;
}
__host__ __device__ __forceinline__ void cl_knn_decode(unsigned long long key, int& row, float& d2) {
    if (key == CL_KNN_EMPTY) { row = -1; d2 = INFINITY; return; }
    const unsigned int b = (unsigned int)(key >> 32);
    row = (int)(unsigned int)(key & 0xFFFFFFFFull);
#ifdef __HIP_DEVICE_COMPILE__
    d2 = __uint_as_float(b);
#else
    memcpy(&d2, &b, 4);
#endif
}

// the K best keys of one lane in registers (K <= KC)
template <int KC>
struct ClKnnReg {
    static constexpr int NT = 256;
    static constexpr int LDS_KEYS = 1;                // no LDS list
    unsigned long long h[KC];
    __device__ __forceinline__ void reset(unsigned long long*, int K) {
#pragma unroll
        for (int u = 0; u < KC; ++u) h[u] = u < KC - K ? 0ull : CL_KNN_EMPTY;
    }
    __device__ __forceinline__ unsigned long long worst() const { return h[KC - 1]; }
    __device__ __forceinline__ void insert(unsigned long long x, int) {      // x < worst()
#pragma unroll
        for (int u = 0; u < KC; ++u) {
            const unsigned long long e = h[u];
            h[u] = e < x ? e : x;
            x = e < x ? x : e;
        }
    }
    __device__ __forceinline__ void write(int K, int* __restrict__ idx, float* __restrict__ d2) {
#pragma unroll
        for (int u = 0; u < KC; ++u) {
            const int r = u - (KC - K);
            if (r >= 0) cl_knn_decode(h[u], idx[r], d2[r]);
        }
    }
};
// ... and in LDS: a max-heap of K keys per lane (K <= KC)
template <int KC>
struct ClKnnHeap {
    static constexpr int NT = 128;
    static constexpr int LDS_KEYS = KC * NT;
    unsigned long long* hp;                           // this lane's column
    unsigned long long top;                           // the root: the worst of the K best so far
    __device__ __forceinline__ void reset(unsigned long long* lds, int K) {
        hp = lds + threadIdx.x;
        for (int r = 0; r < K; ++r) hp[r * NT] = CL_KNN_EMPTY;
        top = CL_KNN_EMPTY;
    }
    __device__ __forceinline__ unsigned long long worst() const { return top; }
    // x takes the root's place in the heap of m entries and sinks to where it belongs
    __device__ __forceinline__ void sift(unsigned long long x, int m) {
        int r = 0;
        for (;;) {
            int c = 2 * r + 1;
            if (c >= m) break;
            unsigned long long a = hp[c * NT];
            if (c + 1 < m) {
                const unsigned long long b = hp[(c + 1) * NT];
                if (b > a) { a = b; ++c; }
            }
            if (a <= x) break;
            hp[r * NT] = a;
            r = c;
        }
        hp[r * NT] = x;
    }
    __device__ __forceinline__ void insert(unsigned long long x, int K) {    // x < worst()
        sift(x, K);
        top = hp[0];
    }
    __device__ __forceinline__ void write(int K, int* __restrict__ idx, float* __restrict__ d2) {
        for (int m = K - 1; m >= 0; --m) {            // heap sort: the largest key leaves for place m, the heap's last entry re-enters at the root
            cl_knn_decode(hp[0], idx[m], d2[m]);
            if (m > 0) sift(hp[m * NT], m);
        }
    }
};

template <typename List>
__global__ __launch_bounds__(List::NT) void k_cl_knn(const float* __restrict__ q, int nq, int qstride, const float4* __restrict__ spts,
                                                     const int* __restrict__ perm, int nt, const ClGrid* __restrict__ gp,
                                                     const int* __restrict__ cs, int K, float max_d2, int* __restrict__ idx,
                                                     float* __restrict__ d2out) {
    constexpr int NT = List::NT;
    __shared__ unsigned int stack[CL_STACK * NT];
    __shared__ unsigned long long keys[List::LDS_KEYS];
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= nq) return;
    const float qx = q[(size_t)i * qstride], qy = q[(size_t)i * qstride + 1], qz = q[(size_t)i * qstride + 2];
    int* const oi = idx + (size_t)i * K;
    float* const od = d2out + (size_t)i * K;
    // a query that is not a point, or no targets at all (then the handle's tables hold nothing): decided before any cell arithmetic
    if (nt == 0 || !(fabsf(qx) < INFINITY && fabsf(qy) < INFINITY && fabsf(qz) < INFINITY)) {
        for (int r = 0; r < K; ++r) { oi[r] = -1; od[r] = INFINITY; }
        return;
    }
    unsigned int* st = stack + threadIdx.x;
    const ClGrid g = *gp;
    const double dx = qx, dy = qy, dz = qz;
    int cx, cy, cz;
    cl_cell_of(g, dx, dy, dz, cx, cy, cz);
    List list;
    list.reset(keys, K);
    const double gate = (double)max_d2;               // +inf arrives as a float32 argument: no 64-bit literal
    double kth = gate;                                // the K-th best d2 so far, exactly; the gate until K targets qualified
    unsigned int wbits = __float_as_uint(max_d2);     // float32 bits of min(gate, K-th best): a candidate above it cannot enter
    const int rx0 = cx >> CL_LMAX, ry0 = cy >> CL_LMAX;
    const int nrx = CL_NX >> CL_LMAX, nry = CL_NY >> CL_LMAX;
    // the query's own root first, then the others; one root's subtree is finished before the next begins (the CL_STACK bound)
    for (int rr = 0; rr < nrx * nry; ++rr) {
        int rx = rr % nrx, ry = rr / nrx;
        if (rr == 0) { rx = rx0; ry = ry0; }
        else if (rx == rx0 && ry == ry0) { rx = 0; ry = 0; }
        st[0] = cl_pack(CL_LMAX, rx, ry, 0);
        int sp = 1;
        while (sp > 0) {
            int l, x, y, z;
            cl_unpack(st[(--sp) * NT], l, x, y, z);
            if (cl_knn_prune_bound(cl_box_d2(g, dx, dy, dz, l, x, y, z)) > kth) continue;      // (the list may have improved since the push)
            const unsigned int c = cl_code(x << l, y << l, z << l) >> (3 * l);
            // the ranges of the node and its eight children: nine consecutive entries of the level below (a cell: its own two ends)
            int bnd[9];
            {
                const long long base = l == 0 ? (long long)CL_NCODES - c
                                     : l == 1 ? (long long)CL_NCODES - 8ll * c
                                              : (long long)(CL_NCODES + 1) + (long long)cl_lvl_off(l - 1) + 8ll * c;
                const long long dir = l <= 1 ? -1 : 1;
#pragma unroll
                for (int u = 0; u < 9; ++u) {
                    const long long at = base + dir * u;
                    bnd[u] = cs[at < 0 ? 0 : at];
                }
            }
            const int j0 = bnd[0], j1 = l == 0 ? bnd[1] : bnd[8];
            if (j0 == j1) continue;
            if (l == 0 || j1 - j0 <= CL_LEAF) {
                for (int jb = j0; jb < j1; jb += 8) {
                    float4 pj[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) pj[u] = spts[jb + u < j1 ? jb + u : j1 - 1];
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const float d2 = cl_d2_f32(qx, qy, qz, pj[u]);
                        // d2 <= gate and d2 <= K-th best in one compare of bit patterns (both are non-negative floats or +inf)
                        if (jb + u >= j1 || __float_as_uint(d2) > wbits) continue;
                        const unsigned long long key = cl_knn_key(d2, perm[jb + u]);
                        if (key >= list.worst()) continue;      // an equal d2 with a higher row
                        list.insert(key, K);
                        const unsigned int wb = (unsigned int)(list.worst() >> 32);
                        if (wb != 0xFFFFFFFFu) { wbits = wb; kth = (double)__uint_as_float(wb); }
                    }
                }
                continue;
            }
            // children, nearest one pushed last (on top); sibling boxes share their faces: two gaps per axis serve all eight
            const int l1 = l - 1;
            const int ox = ((cx >> l1) > 2 * x) ? 1 : 0, oy = ((cy >> l1) > 2 * y) ? 1 : 0, oz = ((cz >> l1) > 2 * z) ? 1 : 0;
            const int near = ox | (oy << 1) | (oz << 2);
            double s2[3][2];
            {
                const int nbx[3] = {CL_NX >> l1, CL_NY >> l1, CL_NZ >> l1};
                const int c2[3] = {2 * x, 2 * y, 2 * z};
                const double q3[3] = {dx, dy, dz}, o3[3] = {g.ox, g.oy, g.oz};
#pragma unroll
                for (int ax = 0; ax < 3; ++ax)
#pragma unroll
                    for (int hb = 0; hb < 2; ++hb) {
                        const double gap = cl_axis_gap(o3[ax], q3[ax], c2[ax] + hb, l1, nbx[ax]);
                        s2[ax][hb] = gap * gap;
                    }
            }
#pragma unroll
            for (int u = 7; u >= 0; --u) {
                const int ch = u ^ near;
                const int hx = ch & 1, hy = (ch >> 1) & 1, hz = (ch >> 2) & 1;
                // the same sum, in the same order, as cl_box_d2 of the child: ((0 + x) + y) + z
                double cd2 = 0.0;
                cd2 += hx ? s2[0][1] : s2[0][0];
                cd2 += hy ? s2[1][1] : s2[1][0];
                cd2 += hz ? s2[2][1] : s2[2][0];
                int lo_i = bnd[0], hi_i = bnd[1];
#pragma unroll
                for (int v = 1; v < 8; ++v) { lo_i = ch == v ? bnd[v] : lo_i; hi_i = ch == v ? bnd[v + 1] : hi_i; }
                const bool keep = lo_i != hi_i && !(cl_knn_prune_bound(cd2) > kth) && sp < CL_STACK;
                st[sp * NT] = cl_pack(l1, 2 * x + hx, 2 * y + hy, 2 * z + hz);      // (slot sp is free: written, kept only if counted)
                sp += keep ? 1 : 0;
            }
        }
    }
    list.write(K, oi, od);
}

template <typename List>
static void cl_launch_knn(vg_cluster* h, const float* d_query, int nq, int qstride, int K, float max_d2, int32_t* d_idx, float* d_d2,
                          hipStream_t st) {
    hipLaunchKernelGGL((k_cl_knn<List>), dim3(vg_div_up(nq, List::NT)), dim3(List::NT), 0, st, d_query, nq, qstride, h->d_spts, h->d_perm,
                       h->grid_n, h->d_grid, h->d_cell_start, K, max_d2, d_idx, d_d2);
}

extern "C" {

int vg_cluster_knn(vg_cluster* h, const float* d_query, int nq, int qstride, int K, float max_d2, int32_t* d_idx, float* d_d2,
                   void* stream) {
    if (!h || nq < 0 || qstride < 3 || K < 1 || K > VG_KNN_MAX_K || !(max_d2 > 0.f)) return VG_ERR_ARG;
    if (nq == 0) return VG_OK;
    if (!d_query || !d_idx || !d_d2) return VG_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (K <= VG_KNN_K_REG1) cl_launch_knn<ClKnnReg<VG_KNN_K_REG1>>(h, d_query, nq, qstride, K, max_d2, d_idx, d_d2, st);
    else if (K <= VG_KNN_K_REG4) cl_launch_knn<ClKnnReg<VG_KNN_K_REG4>>(h, d_query, nq, qstride, K, max_d2, d_idx, d_d2, st);
    else if (K <= VG_KNN_K_REG8) cl_launch_knn<ClKnnReg<VG_KNN_K_REG8>>(h, d_query, nq, qstride, K, max_d2, d_idx, d_d2, st);
    else if (K <= VG_KNN_K_LDS16) cl_launch_knn<ClKnnHeap<VG_KNN_K_LDS16>>(h, d_query, nq, qstride, K, max_d2, d_idx, d_d2, st);
    else cl_launch_knn<ClKnnHeap<VG_KNN_MAX_K>>(h, d_query, nq, qstride, K, max_d2, d_idx, d_d2, st);
    VG_LAUNCH_CHECK();
    return VG_OK;
}

int vg_knn_host(const float* h_query, int nq, int qstride, const float* h_target, int nt, int tstride, int K, float max_d2,
                int32_t* h_idx, float* h_d2) {
    if (nq < 0 || nt < 0 || qstride < 3 || tstride < 3 || K < 1 || K > VG_KNN_MAX_K || !(max_d2 > 0.f)) return VG_ERR_ARG;
    if (nq == 0) return VG_OK;
    if (!h_query || !h_idx || !h_d2 || (nt > 0 && !h_target)) return VG_ERR_ARG;
    for (int i = 0; i < nq; ++i) {
        const float* q = h_query + (size_t)i * qstride;
        unsigned long long best[VG_KNN_MAX_K];        // ascending
        for (int r = 0; r < K; ++r) best[r] = CL_KNN_EMPTY;
        if (std::isfinite(q[0]) && std::isfinite(q[1]) && std::isfinite(q[2]))
            for (int j = 0; j < nt; ++j) {
                const float* t = h_target + (size_t)j * tstride;
                const float d2 = cl_d2_f32(q[0], q[1], q[2], make_float4(t[0], t[1], t[2], 0.f));
                if (!(d2 <= max_d2)) continue;
                unsigned long long x = cl_knn_key(d2, j);
                if (x >= best[K - 1]) continue;
                for (int r = 0; r < K; ++r)
                    if (x < best[r]) std::swap(x, best[r]);
            }
        for (int r = 0; r < K; ++r) cl_knn_decode(best[r], h_idx[(size_t)i * K + r], h_d2[(size_t)i * K + r]);
    }
    return VG_OK;
}

double vg_knn_prune_bound_host(double box_d2) { return cl_knn_prune_bound(box_d2); }

}  // extern "C"
