// Spatial clustering on gfx950 (kernels K2a-K2c): the GPU half of HDBSCAN.
//
// Replaces the work hidden in `cluster_model.fit(points_ref_wo_ground)` (src/vilgod/zero_shot_detector.py:248;
// hdbscan.HDBSCAN(min_cluster_size=15, cluster_selection_epsilon=0.15), tools/configs/preprocessor/waymo.yaml:10-15):
// One translation unit, by stage (each file is included in place, in this order):
//   cluster_geom.inc     the CL_* constants, ClGrid and the __host__ __device__ geometry of the grid and its implicit octree (what
//                        vg_cluster_geom_probe exposes)
//   cluster_grid.inc     K2a  k_cl_bbox / k_cl_grid / k_cl_codes / radix sort / k_cl_gather + min-scan / k_cl_levels (cl_build_grid):
//                        points -> 0.4 m cells, Morton order (6 interleaved bits + 3 high bits of x,y), dense cell-start table and the
//                        same table per coarser level (any 2^l-aligned cube of cells is ONE contiguous range of the sorted points)
//   cluster_core.inc     K2b  k_cl_blocks, k_cl_core_blk, k_cl_core_far (cl_launch_core): exact k-NN core distance in two cooperative
//                        phases over a work list of (octree node, 64 queries) items: A scans the 27 nodes around the item from LDS,
//                        lane = query; B finishes the queries whose k-th distance reaches past that shell, one wave per query, lane =
//                        candidate.  float64 distances; the k smallest live in registers for k <= 15 and in an LDS heap / across the
//                        wave's lanes for 16 <= k <= VG_CLUSTER_MAX_K (see the comment in front of CLB_ORDER)
//   cluster_mst.inc      K2c  k_cl_b_* (cl_mst): exact minimum spanning tree of the mutual-reachability graph, Boruvka rounds over a
//                        pruned depth-first walk of the implicit octree ("nearest point of another component", nearest child first,
//                        box-distance pruning, nodes with <= CL_LEAF points scanned directly): subtrees owned entirely by the query's
//                        component are skipped through per-round purity tables (levels 0..3), and per-component upper bounds
//                        published with atomicMin prune the rest of the component; edges are ordered by the STRICT total order
//                        (w2, pair d2, min id, max id) so the tree is unique and equals the oracle's; radix sort of the n - 1 edges
//                        by weight.  The development build adds dev/cluster_dev.inc from here: the per-point k-NN walk the
//                        cooperative phases replaced, and the A/B switches.
//   cluster_queries.inc  beside the clustering, on the same grid over a TARGET set (vg_cluster_grid): the fixed-radius queries
//                        k_cl_ball_count / k_cl_nearest
//   cluster_ball_query.inc  ... the rows of the targets inside the radius (pcdet's ball_query), k_cl_ball_query: one wave per query
//   cluster_knn.inc      ... and the K nearest targets without a radius, k_cl_knn
//   cluster_dbscan.inc   DBSCAN, the reference's other clustering model, on the same grid: k_db_* (with dbscan_pair.inc)
// This file: the handle -- the counter words (ClCounter), THE list of its buffers (CL_BUFFERS), the buffers DBSCAN borrows
// (ClDbscanView), cl_alloc / create / destroy / vg_cluster_bytes -- and the entry points vg_cluster_grid, vg_cluster_geom_probe,
// vg_cluster_mst[_nd].
// The hierarchy stage (K2d) takes the sorted edges from here: csrc/hdbscan_device.hip on the device, csrc/hdbscan_tree.cpp on the host.
//
// All distances are float64 with d2 = (dx*dx + dy*dy) + dz*dz on exactly converted float32 coordinates
// (what the library computes after its float64 conversion); compiled with -ffp-contract=off.
#include <stddef.h>
#include <string.h>
#include <vector>
#include <algorithm>
#include <cstring>
#include <type_traits>
#include <math.h>
#include "common.h"
#include "vilgod_hip.h"
#include <rocprim/rocprim.hpp>

#include "cluster_geom.inc"

// The words of vg_cluster::d_counter.  The kernels and the host index it by these names only.
enum ClCounter {
    CL_CNT_EDGES = 0,          // MST edges emitted so far (| CL_CYCLE)
    CL_CNT_DONE = 1,           // the tree was complete before this round: every kernel of a round queued ahead returns at once
    CL_CNT_ITEMS = 2,          // work items of the cooperative core-distance phases (k_cl_blocks)
    CL_CNT_FAR = 3,            // queries k_cl_core_blk leaves to k_cl_core_far
    CL_CNT_DEV = 5,            // development build (SEEDSIM)
    CL_CNT_DB_STATUS = 8,      // DBSCAN: not 0 = a bounded walk or retry loop overran (cannot happen)
    CL_CNT_WORDS = 16
};
static_assert(CL_CNT_FAR == CL_CNT_ITEMS + 1, "cl_launch_core clears these two words with one memset");

// THE list of the handle's device buffers, in the order they are allocated: X(member, element type, elements per point of max_points,
// fixed elements, owning stage).  The struct's members, cl_alloc, vg_cluster_destroy and vg_cluster_bytes all come from it.  The stage
// (grid: K2a and the queries; core: K2b; mst: K2c) is not stored: nothing reads it yet -- a grid-only handle would.
#define CL_PUR_TOTAL (cl_pur_off_fwd(CL_PUR_LEVELS))      // entries of a per-node table over levels 0 .. CL_PUR_LEVELS - 1
#define CL_BUFFERS(X) \
    X(d_grid,       ClGrid,             0, 1, grid) \
    X(d_code,       unsigned int,       1, 0, grid)       /* Morton codes, unsorted */ \
    X(d_code_s,     unsigned int,       1, 0, grid)       /* ... sorted */ \
    X(d_perm_in,    int,                1, 0, grid)       /* identity */ \
    X(d_perm,       int,                1, 0, grid)       /* sorted -> original index */ \
    X(d_spts,       float4,             1, 0, grid)       /* sorted points (x,y,z,e): e = 4th clustering coordinate (0 in 3-D) */ \
    X(d_st,         float,              1, 0, grid)       /* sorted 5th clustering coordinate (5-D only) */ \
    X(d_cell_start, int,                0, (size_t)(CL_NCODES + 1) + CL_LVL_TOTAL, grid)   /* reversed min-scan layout (cl_start), then levels 1 .. CL_LMAX (cl_start_l) */ \
    X(d_cell_comp,  int,                0, CL_PUR_TOTAL, mst)       /* purity tables, levels 0..3 back to back: component id if pure, else -1 */ \
    X(d_cell_e,     unsigned int,       0, CL_PUR_TOTAL, grid)      /* same layout: (min, max) of the 4th coordinate in the node as two fp16 (dim >= 4) */ \
    X(d_core2,      double,             1, 0, core)       /* squared core distances, sorted order */ \
    X(d_comp,       int,                1, 0, mst)        /* Boruvka: component (= root) of every point (sorted index space) */ \
    X(d_aux,        int4,               1, 0, mst)        /* per sorted point {core2 (2 words), component, 5th coordinate}: what a leaf scan needs next to spts */ \
    X(d_parent2,    int,                1, 0, mst)        /* this round's hook of every root */ \
    X(d_best_w,     unsigned long long, 1, 0, mst)        /* per component: lightest weight found this round (also the bound the walks prune with) */ \
    X(d_best_e,     unsigned long long, 1, 0, mst)        /* ... its id key */ \
    X(d_sel_a,      int,                1, 0, mst)        /* per component: the two ends of the edge it picked (sel_a = -1: none) */ \
    X(d_sel_b,      int,                1, 0, mst) \
    X(d_pt_w,       unsigned long long, 1, 0, mst)        /* per point: its candidate edge's weight, */ \
    X(d_pt_key,     unsigned long long, 1, 0, mst)        /* ... id key */ \
    X(d_pt_d,       unsigned long long, 1, 0, mst)        /* ... and squared pair distance: the tie-break after w */ \
    X(d_pt_lb,      double,             1, 0, mst)        /* per point: a lower bound of the weight of ANY edge leaving its component (grows over the rounds) */ \
    X(d_best_d,     unsigned long long, 1, 0, mst)        /* per component: the pair distance of its lightest edge */ \
    X(d_pt_b,       int,                1, 0, mst)        /* per point: the other end of its candidate edge, -1: none (kept while it stays foreign: k_cl_b_seed) */ \
    X(d_counter,    int,                0, CL_CNT_WORDS, core)      /* see ClCounter */ \
    X(d_csize,      int,                1, 0, mst)        /* points per component, kept at the component's root (sorted index space) */ \
    X(d_giant,      unsigned long long, 0, 1, mst)        /* this round's largest component: size << 32 | root (0 until the first round's kernels ran) */ \
    X(d_entries,    unsigned int,       1, 0, core)       /* work list of the cooperative phases (k_cl_blocks) */ \
    X(d_far,        int,                1, 0, core)       /* the queries k_cl_core_blk hands on to k_cl_core_far */ \
    X(d_mst_a,      int,                1, 0, mst)        /* the edges' ends, original ids */ \
    X(d_mst_b,      int,                1, 0, mst) \
    X(d_mst_w,      unsigned long long, 1, 0, mst)        /* edge weights as emitted */ \
    X(d_mst_w_s,    unsigned long long, 1, 0, mst)        /* ... sorted */ \
    X(d_mst_idx,    int,                1, 0, mst)        /* edge numbers, carried through the sort */ \
    X(d_mst_idx_s,  int,                1, 0, mst)

struct vg_cluster {
    int max_points;
    int grid_n;                           // points in the grid currently built (vg_cluster_grid / vg_cluster_mst_nd)
#define X(member, T, per_point, fixed, stage) T* member;
    CL_BUFFERS(X)
#undef X
    // not in the list, each for its own reason (cl_alloc):
    void* d_temp;                         // rocprim scratch (sorts, scans): its size is the largest answer of four size queries
    size_t temp_bytes;
    int* h_counter;                       // PINNED HOST memory: the edge count after each of up to 16 queued rounds
    int* d_dbg;                           // only under VG_CLUSTER_DEBUG=1 [max_points]: points scanned per query by the core-distance phases / the last search round
};

struct ClBuf { size_t offset, elem, per_point, fixed; };
static const ClBuf CL_TABLE[] = {
#define X(member, T, per_point, fixed, stage) {offsetof(vg_cluster, member), sizeof(T), per_point, fixed},
    CL_BUFFERS(X)
#undef X
};
static size_t cl_buf_bytes(const ClBuf& b, size_t n) { return b.elem * (b.per_point * n + b.fixed); }
static void** cl_buf_slot(vg_cluster* h, const ClBuf& b) { return (void**)((char*)h + b.offset); }

// DBSCAN (cluster_dbscan.inc) owns no buffer: it works in seven of the Boruvka stage's, int [max_points] each, and one counter word.
// An MST on the handle initialises every one of them that it reads, and so does DBSCAN (k_db_core .. k_db_label write each before its
// first read), so neither sees what the other left.
struct ClDbscanView {
    int *core, *parent, *minrow, *flag, *scan, *root, *label_s;      // [max_points]
    int* status;                                                     // one word
};
static ClDbscanView cl_dbscan_view(vg_cluster* h) {
    static_assert(sizeof(*h->d_comp) == sizeof(int) && sizeof(*h->d_parent2) == sizeof(int) && sizeof(*h->d_csize) == sizeof(int) &&
                  sizeof(*h->d_sel_a) == sizeof(int) && sizeof(*h->d_sel_b) == sizeof(int) && sizeof(*h->d_mst_a) == sizeof(int) &&
                  sizeof(*h->d_pt_b) == sizeof(int), "DBSCAN reads int [max_points] from every lender (one element per point in CL_BUFFERS)");
    ClDbscanView v;
    v.core = h->d_comp;            // lender: the component of every point.   1 = core row
    v.parent = h->d_parent2;       // lender: the round's hooks.              union-find over sorted positions
    v.minrow = h->d_csize;         // lender: the component sizes.            at a root: the component's lowest original row
    v.flag = h->d_sel_a;           // lender: the picked edges' near ends.    original order: 1 at each component's lowest row
    v.scan = h->d_sel_b;           // lender: the picked edges' far ends.     exclusive scan of flag: a component's label
    v.root = h->d_mst_a;           // lender: the emitted edges' first ends.  every core row's root, -1 for the others
    v.label_s = h->d_pt_b;         // lender: the candidates' far ends.       labels in sorted order
    v.status = h->d_counter + CL_CNT_DB_STATUS;
    return v;
}

// VG_CLUSTER_DEBUG=1: the per-query counts of d_dbg once the stream has drained, sorted, with their total and how many are not zero
struct ClDbgCounts {
    std::vector<int> sorted;
    long long total = 0;
    int nonzero = 0;
    int at(int num, int den) const { return sorted[sorted.size() * (size_t)num / (size_t)den]; }      // the num / den quantile
    int max() const { return sorted.back(); }
};
static ClDbgCounts cl_dbg_counts(vg_cluster* h, int n, hipStream_t st) {
    ClDbgCounts c;
    c.sorted.resize(n);
    (void)hipStreamSynchronize(st);
    (void)hipMemcpy(c.sorted.data(), h->d_dbg, 4 * (size_t)n, hipMemcpyDeviceToHost);
    for (int v : c.sorted) { c.total += v; c.nonzero += v > 0; }
    std::sort(c.sorted.begin(), c.sorted.end());
    return c;
}

// body(std::integral_constant<int, dim>): the ONE place that turns the run-time dim (3, 4 or 5) into the kernels' template parameter
template <typename Body>
static int cl_with_dim(int dim, Body&& body) {
    if (dim == 3) return body(std::integral_constant<int, 3>());
    if (dim == 4) return body(std::integral_constant<int, 4>());
    return body(std::integral_constant<int, 5>());
}

#include "cluster_grid.inc"
#include "cluster_core.inc"
#include "cluster_mst.inc"
#include "cluster_queries.inc"
#include "cluster_ball_query.inc"      // the rows inside the radius, pcdet's ball_query: k_cl_ball_query, vg_cluster_ball_query, vg_ball_query_host
#include "cluster_knn.inc"     // K nearest targets, no radius limit: k_cl_knn, vg_cluster_knn, vg_knn_host

// every buffer of a handle whose members are all null (vg_cluster_create frees what is there when this fails half-way)
static int cl_alloc(vg_cluster* h) {
    const size_t n = (size_t)h->max_points;
    for (const ClBuf& b : CL_TABLE) VG_CHECK(hipMalloc(cl_buf_slot(h, b), cl_buf_bytes(b, n)));
    VG_CHECK(hipHostMalloc((void**)&h->h_counter, 64));
    if (getenv("VG_CLUSTER_DEBUG")) VG_CHECK(hipMalloc(&h->d_dbg, 4 * n));
    // the rocprim scratch serves four calls, one at a time: the sort of the Morton codes and the min-scan of the cell table
    // (cl_build_grid), the sort of the edges (cl_mst), and DBSCAN's scan of its flags into its labels (db_run)
    const ClDbscanView db = cl_dbscan_view(h);
    size_t t1 = 0, t2 = 0, t3 = 0, t4 = 0;
    VG_CHECK(rocprim::radix_sort_pairs(nullptr, t1, h->d_code, h->d_code_s, h->d_perm_in, h->d_perm, n, 0, 24));
    VG_CHECK(rocprim::radix_sort_pairs(nullptr, t2, h->d_mst_w, h->d_mst_w_s, h->d_mst_idx, h->d_mst_idx_s, n, 0, 64));
    VG_CHECK(rocprim::inclusive_scan(nullptr, t3, h->d_cell_start, h->d_cell_start, (size_t)(CL_NCODES + 1), MinOp()));
    VG_CHECK(rocprim::exclusive_scan(nullptr, t4, db.flag, db.scan, 0, n, rocprim::plus<int>()));
    h->temp_bytes = std::max(std::max(t1, t4), std::max(t2, t3)) + 256;
    VG_CHECK(hipMalloc(&h->d_temp, h->temp_bytes));
    return VG_OK;
}

extern "C" {

/* HOST ONLY (no HIP call): the bytes of device memory the listed buffers of a handle for max_points points take -- everything but
 * the rocprim scratch and the VG_CLUSTER_DEBUG counts.  0 for max_points <= 0. */
size_t vg_cluster_bytes(int max_points) {
    size_t total = 0;
    if (max_points > 0)
        for (const ClBuf& b : CL_TABLE) total += cl_buf_bytes(b, (size_t)max_points);
    return total;
}

int vg_cluster_create(vg_cluster** out, int max_points) {
    if (!out || max_points <= 0) return VG_ERR_ARG;
    vg_cluster* h = new vg_cluster();
    memset(h, 0, sizeof(*h));
    h->max_points = max_points;
    const int rc = cl_alloc(h);
    if (rc != VG_OK) {
        vg_cluster_destroy(h);
        return rc;
    }
    *out = h;
    return VG_OK;
}

void vg_cluster_destroy(vg_cluster* h) {
    if (!h) return;
    for (const ClBuf& b : CL_TABLE) (void)hipFree(*cl_buf_slot(h, b));
    (void)hipFree(h->d_temp);
    (void)hipFree(h->d_dbg);
    (void)hipHostFree(h->h_counter);
    delete h;
}

/* Builds the 0.4 m cell grid over a TARGET point set (x,y,z = first three columns) for vg_cluster_ball_count /
 * vg_cluster_nearest.  The grid stays valid until the next vg_cluster_grid / vg_cluster_mst[_nd] on this handle. */
int vg_cluster_grid(vg_cluster* h, const float* d_points, int n, int stride, void* stream) {
    if (!h || n < 0 || stride < 3) return VG_ERR_ARG;
    if (n > h->max_points) return VG_ERR_CAPACITY;
    h->grid_n = 0;
    if (n == 0) return VG_OK;
    if (!d_points) return VG_ERR_ARG;
    // (the starting ClGrid is written on the device, as for vg_cluster_dbscan: a copy from this frame's stack, captured into a graph,
    // would be read again at every replay)
    return cl_build_grid(h, d_points, n, stride, 3, (hipStream_t)stream, true);
}

/* HOST ONLY (no GPU): the geometry the walks prune with, evaluated by the functions the kernels call (cl_origin, cl_cell_of,
 * cl_code, cl_box_d2, cl_block_radius2, cl_lvl_off are __host__ __device__).  Pair i = (point i, query i).
 *   h_origin_in [3] f64 or NULL: the origin; NULL: cl_origin of the float32 extremes h_bbox_lo / h_bbox_hi [3]
 *   h_points [n,3] f32 or NULL: NULL reads the cells from h_cell instead of assigning them
 *   h_queries [n,3] f32 or NULL (then h_box_d2 / h_radius2 are not written)
 *   h_origin [3]; h_cell [n,3]; h_code [n]; h_box_d2 [n,7]: cl_box_d2(query i, level-l node of point i's cell), l = 0..6;
 *   h_radius2 [n,7]: cl_block_radius2 of query i around the level-l node of ITS OWN cell; h_lvl_off [8]: cl_lvl_off(l), l = 1..7 ([0] = 0)
 *   (every output may be NULL) */
int vg_cluster_geom_probe(const double* h_origin_in, const float* h_bbox_lo, const float* h_bbox_hi, const float* h_points,
                          const float* h_queries, int n, double* h_origin, int32_t* h_cell, uint32_t* h_code, double* h_box_d2,
                          double* h_radius2, int64_t* h_lvl_off) {
    if (n < 0 || (!h_origin_in && (!h_bbox_lo || !h_bbox_hi)) || (n > 0 && !h_points && !h_cell)) return VG_ERR_ARG;
    ClGrid g;
    memset(&g, 0, sizeof(g));
    g.inf = INFINITY;
    const double ext[3] = {CL_NX * CL_CELL, CL_NY * CL_CELL, CL_NZ * CL_CELL};
    double o[3];
    for (int a = 0; a < 3; ++a) o[a] = h_origin_in ? h_origin_in[a] : cl_origin((double)h_bbox_lo[a], (double)h_bbox_hi[a], ext[a]);
    g.ox = o[0]; g.oy = o[1]; g.oz = o[2];
    if (h_origin) for (int a = 0; a < 3; ++a) h_origin[a] = o[a];
    if (h_lvl_off) {
        h_lvl_off[0] = 0;
        for (int l = 1; l <= CL_LMAX + 1; ++l) h_lvl_off[l] = (int64_t)cl_lvl_off(l);
    }
    const int nb[3] = {CL_NX, CL_NY, CL_NZ};
    for (int i = 0; i < n; ++i) {
        int c[3];
        if (h_points) cl_cell_of(g, (double)h_points[3 * (size_t)i], (double)h_points[3 * (size_t)i + 1], (double)h_points[3 * (size_t)i + 2], c[0], c[1], c[2]);
        else
            for (int a = 0; a < 3; ++a) {
                c[a] = h_cell[3 * (size_t)i + a];
                if (c[a] < 0 || c[a] >= nb[a]) return VG_ERR_ARG;
            }
        if (h_cell && h_points) for (int a = 0; a < 3; ++a) h_cell[3 * (size_t)i + a] = c[a];
        if (h_code) h_code[i] = cl_code(c[0], c[1], c[2]);
        if (!h_queries) continue;
        const double qx = (double)h_queries[3 * (size_t)i], qy = (double)h_queries[3 * (size_t)i + 1], qz = (double)h_queries[3 * (size_t)i + 2];
        int q[3];
        cl_cell_of(g, qx, qy, qz, q[0], q[1], q[2]);
        for (int l = 0; l <= CL_LMAX; ++l) {
            if (h_box_d2) h_box_d2[7 * (size_t)i + l] = cl_box_d2(g, qx, qy, qz, l, c[0] >> l, c[1] >> l, c[2] >> l);
            if (h_radius2) h_radius2[7 * (size_t)i + l] = cl_block_radius2(g, qx, qy, qz, q[0] >> l, q[1] >> l, q[2] >> l, l);
        }
    }
    return VG_OK;
}

}  // extern "C"

extern "C" {

/* Exact core distances + exact MST of the mutual reachability graph.  SYNCHRONOUS on `stream` (one small
 * device->host counter read per Boruvka round).
 *   d_points [n,stride] f32; dim = 3, 4 or 5 leading columns form the clustering space (x,y,z first: the cell grid and
 *   all pruning bounds use x,y,z only -- a lower bound of the dim-D distance; 5-D = the two-frame input of
 *   zero_shot_detector.py:232-237: x,y,z,entropy,0.1*frame).  Distances: float64, summed left to right.
 *   k = min_samples (1 .. VG_CLUSTER_MAX_K): core = distance to the k-th nearest OTHER point (k <= 15: register lists,
 *   k >= 16: ClLdsHeap / the WIDE form of k_cl_core_far)
 *   d_core2  [n] f64 squared core distances, ORIGINAL point order (may be NULL)
 *   d_mst_lo/hi [n-1] int32 original point ids (lo < hi), d_mst_w2 [n-1] f64 squared weights, sorted ascending by
 *   weight (equal weights in unspecified order: vg_hdbscan_tree_host callers sort ties by (lo,hi)).
 *   h_rounds: number of Boruvka rounds (diagnostic, may be NULL). */
int vg_cluster_mst_nd(vg_cluster* h, const float* d_points, int n, int stride, int dim, int k, double* d_core2,
                      int32_t* d_mst_lo, int32_t* d_mst_hi, double* d_mst_w2, int32_t* h_rounds, void* stream) {
    if (!h || !d_points || n < 0 || dim < 3 || dim > 5 || stride < dim || k < 1 || k > VG_CLUSTER_MAX_K) return VG_ERR_ARG;
    if (n > h->max_points) return VG_ERR_CAPACITY;
    if (h_rounds) *h_rounds = 0;
    if (n < 2) return VG_OK;
    return cl_with_dim(dim, [&](auto d) {
        return cl_mst<decltype(d)::value>(h, d_points, n, stride, k, d_core2, d_mst_lo, d_mst_hi, d_mst_w2, h_rounds, (hipStream_t)stream);
    });
}

int vg_cluster_mst(vg_cluster* h, const float* d_points, int n, int stride, int k, double* d_core2, int32_t* d_mst_lo,
                   int32_t* d_mst_hi, double* d_mst_w2, int32_t* h_rounds, void* stream) {
    return vg_cluster_mst_nd(h, d_points, n, stride, 3, k, d_core2, d_mst_lo, d_mst_hi, d_mst_w2, h_rounds, stream);
}

}  // extern "C"

#include "dbscan_pair.inc"         // the DBSCAN pair test, __host__ __device__
#include "cluster_dbscan.inc"      // DBSCAN on the grid: k_db_*, vg_cluster_dbscan, vg_dbscan_host
