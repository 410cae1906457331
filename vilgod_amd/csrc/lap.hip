// Batched linear assignment for gfx950: the device counterpart of scipy.optimize.linear_sum_assignment, which the reference calls in
// src/datasets/waymo_eval.py:111 (through the metric's matcher) and src/utils/tracking_utils.py:23-51.
//
//   k_lap_groups  one WAVE per group, 16 or 4 independent waves per workgroup, no workgroup barrier (the groups' trip counts differ).
//                 Shortest augmenting paths with duals, one row at a time in the caller's order, so the state after the k-th row is an
//                 optimal assignment of the first k rows: a snapshot of col4row is written at every prefix length the caller lists.
//     columns     j -> lane j % 64.  v, path cost, predecessor and row4col of a group of at most LAP_REG_COLS = 256 columns live in
//                 registers (4 per lane: 24 VGPRs of state, which leaves the kernel far below the 128 at which a SIMD loses waves; the
//                 evaluation's groups are tens of columns wide); a wider group keeps them in the wave's LDS slice.  The visited bit is
//                 one bit per slot of a lane's 16-bit mask in both forms.  The wave picks its form by its own group's width.
//     rows        u and col4row are read by the (wave-uniform) current row: they live in the wave's LDS slice in both forms.
//     step        the current row of the matrix is read coalesced, every lane relaxes its columns (csrc/lap_step.inc) and the arg-min
//                 over the (cost, free-first, column) key is one xor butterfly.  "Stay unassigned" needs no columns: a row's private
//                 column can only be a sink, so one running minimum over the rows visited in the search stands for all of them.
//     finish      the dual updates are lane-parallel (every visited column owns a different row); the augmentation walks the path, one
//                 wave-uniform step per edge.
// The LDS slices are dynamic, sized from max_rows / max_cols; the grid from n_groups: nothing is read back.  vg_lap_groups_host runs the
// same steps over host arrays, one column after the other.
#include <vector>
#include "common.h"
#include "vilgod_hip.h"
#include "lap_step.inc"

#define LAP_WAVES_MAX 16          // waves per workgroup while their slices fit 64 KiB of LDS (every register-form call of up to 256 rows) ...
#define LAP_WAVES_MIN 4           // ... and beyond that (4 x 36 KiB at the size limit)
#define LAP_REG_SLOTS 4
#define LAP_REG_COLS (64 * LAP_REG_SLOTS)

// ---- what both forms read from the tables ------------------------------------------------------------------------------------
// status -1 with fill_n entries to fill per reachable snapshot, or status 0 and the group's geometry
struct LapGroup {
    int n, m, row0, p0, p1, status, fill_n;
    int64_t cost0;
};

LAP_HD LapGroup lap_group(int g, const int64_t* cost_off, const int32_t* row_off, const int32_t* col_off, const int32_t* prefix_off,
                          bool ordered, int64_t cost_len, int n_rows, int n_snaps, int max_rows, int max_cols) {
    LapGroup G;
    const int64_t r0 = row_off[g], n = (int64_t)row_off[g + 1] - r0, m = (int64_t)col_off[g + 1] - col_off[g];
    G.cost0 = cost_off[g];
    G.row0 = (int)r0;
    G.p0 = prefix_off ? prefix_off[g] : g;
    G.p1 = prefix_off ? prefix_off[g + 1] : g + 1;
    G.status = 0;
    if (G.p0 < 0 || G.p1 < G.p0 || G.p1 > n_snaps) { G.status = -1; G.p0 = G.p1 = 0; }     // no snapshot can be located
    if (n < 0 || m < 0 || n > max_rows || m > max_cols) G.status = -1;
    G.fill_n = (int)(n < 0 ? 0 : n > max_rows ? max_rows : n);
    G.n = G.fill_n;
    G.m = (int)(m < 0 ? 0 : m > max_cols ? max_cols : m);
    if (G.status == 0 && (G.cost0 < 0 || G.cost0 + n * m > cost_len)) G.status = -1;
    if (G.status == 0 && ordered && (r0 < 0 || r0 + n > n_rows)) G.status = -1;
    return G;
}

// snapshot s of a group of n rows: its prefix length (prev: the one before, 0 for the first) and its place in d_match
LAP_HD bool lap_snapshot_ok(bool listed, int len, int prev, int n, int64_t at, int64_t match_len) {
    return (!listed || (len > prev && len <= n)) && at >= 0 && at + n <= match_len;
}

// ---- the kernel -----------------------------------------------------------------------------------------------------------
// LDS hand-offs are between the lanes of ONE wave, whose LDS operations complete in order; the fence pair keeps the compiler from
// moving them across (no instruction is emitted for it)
__device__ __forceinline__ void lap_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct LapSlice {
    double *u, *v, *sh;
    int *c4r, *pred, *r4c;
};

// a wave's per-column state: registers (REG) or its LDS slice.  Slot k of lane l is column l + 64 k; REG loops are unrolled, so the
// arrays are indexed by constants only.
template <bool REG>
struct LapCols {
    double v_[REG ? LAP_REG_SLOTS : 1], sh_[REG ? LAP_REG_SLOTS : 1];
    int pred_[REG ? LAP_REG_SLOTS : 1], r4c_[REG ? LAP_REG_SLOTS : 1];
    LapSlice s;
    int lane;
    __device__ __forceinline__ double& v(int k) { if constexpr (REG) return v_[k]; else return s.v[lane + 64 * k]; }
    __device__ __forceinline__ double& sh(int k) { if constexpr (REG) return sh_[k]; else return s.sh[lane + 64 * k]; }
    __device__ __forceinline__ int& pred(int k) { if constexpr (REG) return pred_[k]; else return s.pred[lane + 64 * k]; }
    __device__ __forceinline__ int& r4c(int k) { if constexpr (REG) return r4c_[k]; else return s.r4c[lane + 64 * k]; }
    // a field of the (wave-uniform) column j, for every lane
    __device__ __forceinline__ int uniform_of(const int (&a)[REG ? LAP_REG_SLOTS : 1], const int* lds, int j) {
        if constexpr (REG) {
            switch (j >> 6) {                                // (a select chain over a[k] is turned into an indexed read: scratch)
                case 0: return __builtin_amdgcn_readlane(a[0], j & 63);
                case 1: return __builtin_amdgcn_readlane(a[1], j & 63);
                case 2: return __builtin_amdgcn_readlane(a[2], j & 63);
                default: return __builtin_amdgcn_readlane(a[3], j & 63);
            }
        } else {
            return lds[j];
        }
    }
    __device__ __forceinline__ int pred_of(int j) { return uniform_of(pred_, s.pred, j); }
    __device__ __forceinline__ int r4c_of(int j) { return uniform_of(r4c_, s.r4c, j); }
    __device__ __forceinline__ void set_r4c(int j, int i) {
        if constexpr (REG) {
#pragma unroll
            for (int k = 0; k < LAP_REG_SLOTS; ++k) r4c_[k] = (j == lane + 64 * k) ? i : r4c_[k];
        } else {
            s.r4c[j] = i;                                    // every lane, one address, one value
        }
    }
};

// -> 0 solved, 1 infeasible.  Snapshots p0 .. p1 - 1 are written as their prefix lengths are reached (tables already checked).
template <bool REG>
__device__ __forceinline__ int lap_solve_wave(const double* __restrict__ cost, int n, int m, double unassigned, const int32_t* order,
                                              const int32_t* prefix, int p0, int p1, const int64_t* __restrict__ match_off,
                                              int32_t* __restrict__ match, LapSlice s, int lane) {
    LapCols<REG> C;
    C.s = s;
    C.lane = lane;
    const int slots = REG ? LAP_REG_SLOTS : (m + 63) >> 6;
#pragma unroll
    for (int k = 0; k < slots; ++k) {
        if (REG || lane + 64 * k < m) { C.v(k) = 0.0; C.r4c(k) = -1; }
    }
    for (int e = lane; e < n; e += 64) { s.u[e] = 0.0; s.c4r[e] = -1; }
    lap_wave_sync();
    int next = p0;
    for (int step = 0; step < n; ++step) {
        const int cur = vg_uniform(order ? order[step] : step);
#pragma unroll
        for (int k = 0; k < slots; ++k) {
            if (REG || lane + 64 * k < m) { C.sh(k) = INFINITY; C.pred(k) = -1; }
        }
        unsigned done = 0;
        int i = cur, drow = -1, sink = -1;                  // sink: a column, or m for "row drow stays unassigned"
        double minv = 0.0, dmin = INFINITY;
        for (;;) {
            const double ui = s.u[i];
            lap_unassigned_best(lap_unassigned_offer(minv, unassigned, ui), i, dmin, drow);
            const double* __restrict__ row = cost + (int64_t)i * m;
            double bc = INFINITY;
            int bt = LAP_TAG_NONE;
#pragma unroll
            for (int k = 0; k < slots; ++k) {
                const int j = lane + 64 * k;
                if (j < m && !((done >> k) & 1u)) {
                    double sh = C.sh(k);
                    int pr = C.pred(k);
                    lap_relax(minv, row[j], ui, C.v(k), i, sh, pr);
                    C.sh(k) = sh;
                    C.pred(k) = pr;
                    const int tag = lap_tag(C.r4c(k) >= 0, j);
                    if (lap_key_less(sh, tag, bc, bt)) { bc = sh; bt = tag; }
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const double oc = __shfl_xor(bc, o);
                const int ot = __shfl_xor(bt, o);
                if (lap_key_less(oc, ot, bc, bt)) { bc = oc; bt = ot; }
            }
            bc = vg_uniform(bc);
            bt = vg_uniform(bt);
            if (!(bc < INFINITY) && !(dmin < INFINITY)) return 1;
            if (lap_key_less(dmin, lap_tag(false, m + drow), bc, bt)) { minv = dmin; sink = m; break; }
            const int j = lap_tag_col(bt);
            minv = bc;
            if (lane == (j & 63)) done |= 1u << (j >> 6);
            if (!lap_tag_assigned(bt)) { sink = j; break; }
            if (!REG) lap_wave_sync();
            i = vg_uniform(C.r4c_of(j));
        }
        // duals: the new row, then every visited column but the sink with the row it holds (all different rows)
        if (lane == 0) s.u[cur] = s.u[cur] + minv;
#pragma unroll
        for (int k = 0; k < slots; ++k) {
            const int j = lane + 64 * k;
            if (j < m && ((done >> k) & 1u) && j != sink) {
                const int r = C.r4c(k);
                double ur = s.u[r], vj = C.v(k);
                lap_dual(minv, C.sh(k), ur, vj);
                s.u[r] = ur;
                C.v(k) = vj;
            }
        }
        lap_wave_sync();
        // augment along the predecessors, from the sink back to the new row
        int j = sink;
        bool open = true;
        if (sink == m) {
            const int jn = s.c4r[drow];
            lap_wave_sync();
            s.c4r[drow] = -1;
            open = drow != cur;
            j = vg_uniform(jn);
        }
        while (open) {
            const int pi = vg_uniform(C.pred_of(j));
            C.set_r4c(j, pi);
            const int jn = s.c4r[pi];
            lap_wave_sync();
            s.c4r[pi] = j;
            open = pi != cur;
            j = vg_uniform(jn);
        }
        lap_wave_sync();
        if (next < p1 && (prefix ? prefix[next] : n) == step + 1) {
            int32_t* out = match + match_off[next];
            for (int e = lane; e < n; e += 64) out[e] = s.c4r[e];
            ++next;
        }
    }
    return 0;
}

__global__ __launch_bounds__(64 * LAP_WAVES_MAX) void k_lap_groups(const double* __restrict__ cost, int64_t cost_len,
                                                               const int64_t* __restrict__ cost_off, const int32_t* __restrict__ row_off,
                                                               const int32_t* __restrict__ col_off, int n_groups, int n_rows, int max_rows,
                                                               int max_cols, double unassigned, const int32_t* __restrict__ order,
                                                               const int32_t* __restrict__ prefix, const int32_t* __restrict__ prefix_off,
                                                               int n_snaps, const int64_t* __restrict__ match_off, int64_t match_len,
                                                               int32_t* __restrict__ match, int32_t* __restrict__ status, int lds_rows,
                                                               int lds_cols) {
    extern __shared__ double lap_lds[];
    const int lane = threadIdx.x & 63, wave = vg_uniform((int)(threadIdx.x >> 6));
    const int waves = blockDim.x >> 6;
    const int g = blockIdx.x * waves + wave;
    if (g >= n_groups) return;
    LapSlice s;
    {
        const int per_wave = lds_rows + 2 * lds_cols;        // doubles, then as many ints
        double* d = lap_lds + (size_t)wave * per_wave;
        int* q = (int*)(lap_lds + (size_t)waves * per_wave) + (size_t)wave * per_wave;
        s.u = d; s.v = d + lds_rows; s.sh = s.v + lds_cols;
        s.c4r = q; s.pred = q + lds_rows; s.r4c = s.pred + lds_cols;
    }
    LapGroup G = lap_group(g, cost_off, row_off, col_off, prefix_off, order != nullptr, cost_len, n_rows, n_snaps, max_rows, max_cols);
    const int n = G.n, m = G.m;
    int st = G.status;
    // the snapshots' lengths and places
    if (st == 0) {
        bool bad = false;
        for (int t = G.p0 + lane; t < G.p1; t += 64) {
            const int len = prefix ? prefix[t] : n, prev = prefix && t > G.p0 ? prefix[t - 1] : 0;
            bad |= !lap_snapshot_ok(prefix != nullptr, len, prev, n, match_off[t], match_len);
        }
        if (__any(bad)) st = -1;
    }
    // the order: in range, and every row once (c4r as the mark: the last writer of a row's mark is the only one that finds itself)
    const int32_t* ord = order ? order + G.row0 : nullptr;
    if (st == 0 && ord) {
        bool bad = false;
        for (int e = lane; e < n; e += 64) {
            const int o = ord[e];
            if (o < 0 || o >= n) bad = true; else s.c4r[o] = e;
        }
        lap_wave_sync();
        for (int e = lane; e < n; e += 64) {
            const int o = ord[e];
            if (o >= 0 && o < n && s.c4r[o] != e) bad = true;
        }
        lap_wave_sync();
        if (__any(bad)) st = -1;
    }
    // the entries
    if (st == 0) {
        bool bad = false;
        const double* c = cost + G.cost0;
        for (int64_t e = lane; e < (int64_t)n * m; e += 64) bad |= lap_invalid(c[e]);
        if (__any(bad)) st = 2;
    }
    if (st == 0) {
        if (m <= LAP_REG_COLS)
            st = lap_solve_wave<true>(cost + G.cost0, n, m, unassigned, ord, prefix, G.p0, G.p1, match_off, match, s, lane);
        else
            st = lap_solve_wave<false>(cost + G.cost0, n, m, unassigned, ord, prefix, G.p0, G.p1, match_off, match, s, lane);
    }
    if (st != 0) {
        for (int t = G.p0; t < G.p1; ++t) {
            const int64_t at = match_off[t];
            if (at < 0 || at + G.fill_n > match_len) continue;
            for (int e = lane; e < G.fill_n; e += 64) match[at + e] = -1;
        }
    }
    if (lane == 0) status[g] = st;
}

static int lap_check_call(const void* cost, int64_t cost_len, const void* cost_off, const void* row_off, const void* col_off, int n_groups,
                          int n_rows, int max_rows, int max_cols, double unassigned, const void* prefix, const void* prefix_off,
                          int n_snaps, const void* match_off, int64_t match_len, const void* match, const void* status) {
    if (n_groups < 0 || n_rows < 0 || n_snaps < 0 || cost_len < 0 || match_len < 0) return VG_ERR_ARG;
    if (max_rows < 0 || max_cols < 0 || max_rows > VG_LAP_MAX || max_cols > VG_LAP_MAX) return VG_ERR_ARG;
    if (!(unassigned == unassigned) || unassigned == -INFINITY) return VG_ERR_ARG;
    if ((prefix == nullptr) != (prefix_off == nullptr)) return VG_ERR_ARG;
    if (!prefix && n_snaps != n_groups) return VG_ERR_ARG;
    if (n_groups == 0) return VG_OK;
    if (!cost_off || !row_off || !col_off || !status) return VG_ERR_ARG;
    if (n_snaps > 0 && !match_off) return VG_ERR_ARG;
    if (cost_len > 0 && !cost) return VG_ERR_ARG;
    if (match_len > 0 && !match) return VG_ERR_ARG;
    return VG_OK;
}

extern "C" int vg_lap_groups(const double* d_cost, int64_t cost_len, const int64_t* d_cost_off, const int32_t* d_row_off,
                             const int32_t* d_col_off, int n_groups, int n_rows, int max_rows, int max_cols, double unassigned_cost,
                             const int32_t* d_order, const int32_t* d_prefix, const int32_t* d_prefix_off, int n_snaps,
                             const int64_t* d_match_off, int64_t match_len, int32_t* d_match, int32_t* d_status, void* stream) {
    const int rc = lap_check_call(d_cost, cost_len, d_cost_off, d_row_off, d_col_off, n_groups, n_rows, max_rows, max_cols,
                                  unassigned_cost, d_prefix, d_prefix_off, n_snaps, d_match_off, match_len, d_match, d_status);
    if (rc != VG_OK || n_groups == 0) return rc;
    const int lds_rows = (max_rows + 1) & ~1, lds_cols = max_cols > LAP_REG_COLS ? (max_cols + 1) & ~1 : 0;
    const size_t per_wave = (size_t)(lds_rows + 2 * lds_cols) * 12;
    const int waves = per_wave * LAP_WAVES_MAX <= 65536 ? LAP_WAVES_MAX : LAP_WAVES_MIN;
    const size_t lds = waves * per_wave;
    VG_MAX_DYNAMIC_LDS(k_lap_groups, LAP_WAVES_MIN * (VG_LAP_MAX * 3) * 12);
    hipLaunchKernelGGL(k_lap_groups, dim3(vg_div_up(n_groups, waves)), dim3(64 * waves), lds, (hipStream_t)stream, d_cost,
                       cost_len, d_cost_off, d_row_off, d_col_off, n_groups, n_rows, max_rows, max_cols, unassigned_cost, d_order, d_prefix,
                       d_prefix_off, n_snaps, d_match_off, match_len, d_match, d_status, lds_rows, lds_cols);
    VG_LAUNCH_CHECK();
    return VG_OK;
}

// ---- the host form ------------------------------------------------------------------------------------------------------------
static int lap_solve_host(const double* cost, int n, int m, double unassigned, const int32_t* order, const int32_t* prefix, int p0,
                          int p1, const int64_t* match_off, int32_t* match) {
    std::vector<double> u(n, 0.0), v(m, 0.0), sh(m);
    std::vector<int> c4r(n, -1), r4c(m, -1), pred(m);
    std::vector<char> done(m);
    int next = p0;
    for (int step = 0; step < n; ++step) {
        const int cur = order ? order[step] : step;
        for (int j = 0; j < m; ++j) { sh[j] = INFINITY; pred[j] = -1; done[j] = 0; }
        int i = cur, drow = -1, sink = -1;
        double minv = 0.0, dmin = INFINITY;
        for (;;) {
            const double ui = u[i];
            lap_unassigned_best(lap_unassigned_offer(minv, unassigned, ui), i, dmin, drow);
            const double* row = cost + (int64_t)i * m;
            double bc = INFINITY;
            int bt = LAP_TAG_NONE;
            for (int j = 0; j < m; ++j) {
                if (done[j]) continue;
                lap_relax(minv, row[j], ui, v[j], i, sh[j], pred[j]);
                const int tag = lap_tag(r4c[j] >= 0, j);
                if (lap_key_less(sh[j], tag, bc, bt)) { bc = sh[j]; bt = tag; }
            }
            if (!(bc < INFINITY) && !(dmin < INFINITY)) return 1;
            if (lap_key_less(dmin, lap_tag(false, m + drow), bc, bt)) { minv = dmin; sink = m; break; }
            const int j = lap_tag_col(bt);
            minv = bc;
            done[j] = 1;
            if (!lap_tag_assigned(bt)) { sink = j; break; }
            i = r4c[j];
        }
        u[cur] = u[cur] + minv;
        for (int j = 0; j < m; ++j)
            if (done[j] && j != sink) lap_dual(minv, sh[j], u[r4c[j]], v[j]);
        int j = sink;
        bool open = true;
        if (sink == m) {
            const int jn = c4r[drow];
            c4r[drow] = -1;
            open = drow != cur;
            j = jn;
        }
        while (open) {
            const int pi = pred[j];
            r4c[j] = pi;
            const int jn = c4r[pi];
            c4r[pi] = j;
            open = pi != cur;
            j = jn;
        }
        if (next < p1 && (prefix ? prefix[next] : n) == step + 1) {
            int32_t* out = match + match_off[next];
            for (int e = 0; e < n; ++e) out[e] = c4r[e];
            ++next;
        }
    }
    return 0;
}

extern "C" int vg_lap_groups_host(const double* h_cost, int64_t cost_len, const int64_t* h_cost_off, const int32_t* h_row_off,
                                  const int32_t* h_col_off, int n_groups, int n_rows, int max_rows, int max_cols, double unassigned_cost,
                                  const int32_t* h_order, const int32_t* h_prefix, const int32_t* h_prefix_off, int n_snaps,
                                  const int64_t* h_match_off, int64_t match_len, int32_t* h_match, int32_t* h_status) {
    const int rc = lap_check_call(h_cost, cost_len, h_cost_off, h_row_off, h_col_off, n_groups, n_rows, max_rows, max_cols,
                                  unassigned_cost, h_prefix, h_prefix_off, n_snaps, h_match_off, match_len, h_match, h_status);
    if (rc != VG_OK || n_groups == 0) return rc;
    for (int g = 0; g < n_groups; ++g) {
        const LapGroup G = lap_group(g, h_cost_off, h_row_off, h_col_off, h_prefix_off, h_order != nullptr, cost_len, n_rows, n_snaps, max_rows, max_cols);
        const int n = G.n, m = G.m;
        int st = G.status;
        for (int t = G.p0; st == 0 && t < G.p1; ++t) {
            const int len = h_prefix ? h_prefix[t] : n, prev = h_prefix && t > G.p0 ? h_prefix[t - 1] : 0;
            if (!lap_snapshot_ok(h_prefix != nullptr, len, prev, n, h_match_off[t], match_len)) st = -1;
        }
        const int32_t* ord = h_order ? h_order + G.row0 : nullptr;
        if (st == 0 && ord) {
            std::vector<char> seen(n, 0);
            for (int e = 0; e < n && st == 0; ++e) {
                const int o = ord[e];
                if (o < 0 || o >= n || seen[o]) st = -1; else seen[o] = 1;
            }
        }
        if (st == 0) {
            const double* c = h_cost + G.cost0;
            for (int64_t e = 0; e < (int64_t)n * m && st == 0; ++e)
                if (lap_invalid(c[e])) st = 2;
        }
        if (st == 0) st = lap_solve_host(h_cost + G.cost0, n, m, unassigned_cost, ord, h_prefix, G.p0, G.p1, h_match_off, h_match);
        if (st != 0) {
            for (int t = G.p0; t < G.p1; ++t) {
                const int64_t at = h_match_off[t];
                if (at < 0 || at + G.fill_n > match_len) continue;
                for (int e = 0; e < G.fill_n; ++e) h_match[at + e] = -1;
            }
        }
        h_status[g] = st;
    }
    return VG_OK;
}
