// Part of cluster.hip (included in place, behind cluster_queries.inc): the INDEX form of the fixed-radius query -- k_cl_ball_query and
// its entry points vg_cluster_ball_query / vg_ball_query_host.  pcdet's `pointnet2_stack.pointnet2_utils.ball_query`
// (ball_query_kernel_stack plus its Python wrapper) as the reference calls it in src/utils/pointcloud_utils.py:83 and :99; the
// definition is in include/vilgod_hip.h.  Expects cluster_geom.inc, cluster_queries.inc (cl_d2_f32, cl_cell_d2_lb) and vg_cluster.
//
// pcdet walks the targets in ROW order and keeps the first nsample hits.  The grid meets them in CELL order, so the kernel has to see
// every hit of the ball and keep the nsample lowest rows; it cannot stop at the cap as k_cl_ball_count does.
//
// One WAVE per query, CL_BQ_WAVES independent waves per workgroup:
//   cells     the reach cube ((2 reach + 1)^3 cells, clipped by the grid), 64 cells per round, one per lane; a lane drops its cell by
//             cl_cell_d2_lb exactly as k_cl_ball_count does.  A wave prefix sum over the surviving ranges flattens them into ONE
//             candidate list per round, and the lanes stride over its points (a binary search over the 64 prefix values, by lane
//             shuffles, finds a candidate's cell): no lane idles over the mostly empty cells of a large reach.
//   hits      rows (perm[j]) are appended to the wave's LDS buffer of VG_BALL_QUERY_CAND entries by ballot and lane prefix.
//   the cut   before a batch of 64 candidates could overflow the buffer (held > CAND - 64) it is sorted (bitonic, in LDS), the nsample
//             smallest rows stay and the largest of them becomes the threshold: from then on only hits BELOW it are appended.  A row
//             dropped by the cut or by the threshold is never among the nsample smallest, because nsample smaller ones were held.
//             CAND - 64 >= nsample, so the cut always makes room.
//   output    what is held is sorted once more; the whole wave writes cnt rows and the padding with coalesced stores.
// The order in which cells and points are met decides the number of sorts only, never the result: the same bits on every run.
//
// No workgroup barrier anywhere: the waves of a workgroup serve different queries with different trip counts.  The LDS hand-offs are
// between the lanes of ONE wave, whose LDS operations are issued and completed in order; what is needed is that the compiler keeps
// that order, which cl_bq_wave_sync gives (a wavefront-scope release / acquire fence pair around a wave barrier: no instruction,
// and no LDS access moves across it).  (k_cl_core_far keeps its list across the 64 lanes in registers and hands values over by readlane; 2 048 rows do not
// fit there, the prefix values and range starts of a round do and are handed over the same way.)  Every loop is bounded by the cell
// ranges or by the buffer size; there is no retry and no spin, no global atomic, nothing read back, nothing allocated.

#define CL_BQ_WAVES 4
#define CL_BQ_EMPTY 0x7FFFFFFF      // behind every row in the sort; as a threshold: none yet
static_assert((VG_BALL_QUERY_CAND & (VG_BALL_QUERY_CAND - 1)) == 0 && VG_BALL_QUERY_CAND >= 128, "the bitonic sort takes a power of two, whole batches of 64 pairs");
static_assert(VG_BALL_QUERY_CAND >= 2 * VG_BALL_QUERY_MAX_NSAMPLE && VG_BALL_QUERY_CAND - 64 >= VG_BALL_QUERY_MAX_NSAMPLE,
              "after a cut at least half the buffer is free, and a batch of 64 fits");

__device__ __forceinline__ void cl_bq_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// buf[held, P) = CL_BQ_EMPTY, then buf[0, P) ascending: a bitonic network over the 64 lanes of one wave.  P: a power of two,
// 128 <= P <= VG_BALL_QUERY_CAND, so every lane takes P / 128 pairs of every step (wave-uniform trip counts).
__device__ __forceinline__ void cl_bq_sort(int* buf, int held, int P, int lane) {
    for (int s = held + lane; s < P; s += 64) buf[s] = CL_BQ_EMPTY;
    cl_bq_wave_sync();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = lane; t < (P >> 1); t += 64) {
                const int i = 2 * t - (t & (j - 1));          // bit j of i is clear: the pair (i, i + j); each entry is in one pair
                const int a = buf[i], b = buf[i + j];
                const bool up = (i & k) == 0;
                if ((a > b) == up) { buf[i] = b; buf[i + j] = a; }
            }
            cl_bq_wave_sync();
        }
}

__global__ __launch_bounds__(64 * CL_BQ_WAVES) void k_cl_ball_query(const float* __restrict__ q, int nq, int qstride,
                                                                    const float4* __restrict__ spts, const int* __restrict__ perm, int nt,
                                                                    const ClGrid* __restrict__ gp, const int* __restrict__ cs, float r2,
                                                                    int reach, int nsample, int* __restrict__ idx, int* __restrict__ cnt_out) {
    __shared__ int rows[CL_BQ_WAVES * VG_BALL_QUERY_CAND];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // (the query is wave-uniform: say so)
    const int i = blockIdx.x * CL_BQ_WAVES + wave;
    if (i >= nq) return;
    int* const buf = rows + wave * VG_BALL_QUERY_CAND;
    const float qx = q[(size_t)i * qstride], qy = q[(size_t)i * qstride + 1], qz = q[(size_t)i * qstride + 2];
    int held = 0;                                             // rows in buf (wave-uniform, as thr)
    int thr = CL_BQ_EMPTY;                                    // only rows below it can still be among the nsample smallest
    // a query that is not a point, or no targets at all (then the handle's tables hold nothing): an empty ball, decided before any cell
    // arithmetic
    if (nt != 0 && fabsf(qx) < INFINITY && fabsf(qy) < INFINITY && fabsf(qz) < INFINITY) {
        const ClGrid g = *gp;
        int cx, cy, cz;
        cl_cell_of(g, qx, qy, qz, cx, cy, cz);
        cx = __builtin_amdgcn_readfirstlane(cx); cy = __builtin_amdgcn_readfirstlane(cy); cz = __builtin_amdgcn_readfirstlane(cz);
        const int x0 = max(cx - reach, 0), y0 = max(cy - reach, 0), z0 = max(cz - reach, 0);
        const int wx = min(cx + reach, CL_NX - 1) - x0 + 1, wy = min(cy + reach, CL_NY - 1) - y0 + 1, wz = min(cz + reach, CL_NZ - 1) - z0 + 1;
        const int ncell = wx * wy * wz;                       // <= 17^3
        for (int cb = 0; cb < ncell; cb += 64) {
            const int c = cb + lane;
            int j0 = 0, n = 0;                                // this lane's cell: its range of sorted points (none: dropped or no cell)
            if (c < ncell) {
                const int x = x0 + c % wx, y = y0 + (c / wx) % wy, z = z0 + c / (wx * wy);
                if (!(cl_cell_d2_lb(g, qx, qy, qz, x, y, z) >= r2)) {           // (>= r2: no point of this cell can be inside)
                    const unsigned int code = cl_code(x, y, z);
                    j0 = cl_start(cs, code);
                    n = cl_start(cs, code + 1u) - j0;
                }
            }
            int inc = n;                                      // inclusive prefix sum over the lanes
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int v = __shfl_up(inc, d);
                inc += lane >= d ? v : 0;
            }
            const int excl = inc - n, total = __builtin_amdgcn_readlane(inc, 63);
            for (int tb = 0; tb < total; tb += 64) {
                if (held > VG_BALL_QUERY_CAND - 64) {         // the next batch might not fit: the cut
                    cl_bq_sort(buf, held, VG_BALL_QUERY_CAND, lane);
                    held = nsample;
                    thr = __builtin_amdgcn_readfirstlane(buf[nsample - 1]);
                }
                const int t = tb + lane;
                // the cell of candidate t: the last lane whose exclusive prefix is <= t (its range is not empty and holds t)
                int lo = 0;
#pragma unroll
                for (int s = 32; s > 0; s >>= 1) {
                    const int v = __shfl(excl, lo + s);
                    lo += v <= t ? s : 0;
                }
                const int j = __shfl(j0, lo) + (t - __shfl(excl, lo));
                bool hit = false;
                int row = 0;
                if (t < total && cl_d2_f32(qx, qy, qz, spts[j]) < r2) {
                    row = perm[j];
                    hit = row < thr;
                }
                const unsigned long long m = __ballot(hit);
                if (hit) buf[held + __popcll(m & ((1ull << lane) - 1ull))] = row;
                held += __popcll(m);
            }
        }
    }
    const int cnt = min(held, nsample);
    if (held > 0) {
        int P = 128;
        while (P < held) P <<= 1;
        cl_bq_sort(buf, held, P, lane);
    }
    int* const orow = idx + (size_t)i * nsample;
    for (int s = lane; s < nsample; s += 64) {                // pcdet pads with the first hit; an empty ball: zeros
        const int v = buf[s < cnt ? s : 0];
        orow[s] = cnt > 0 ? v : 0;
    }
    if (cnt_out && lane == 0) cnt_out[i] = cnt;
}

extern "C" {

int vg_cluster_ball_query(vg_cluster* h, const float* d_query, int nq, int qstride, float r2, int nsample, int32_t* d_idx,
                          int32_t* d_cnt, void* stream) {
    if (!h || nq < 0 || qstride < 3 || !(r2 > 0.f) || nsample < 1 || nsample > VG_BALL_QUERY_MAX_NSAMPLE) return VG_ERR_ARG;
    const double cells = ceil(sqrt((double)r2) / CL_CELL);        // (compared as a double: +inf has no int)
    if (!(cells <= 8.0)) return VG_ERR_ARG;
    const int reach = (int)cells;
    if (nq == 0) return VG_OK;
    if (!d_query || !d_idx) return VG_ERR_ARG;
    hipLaunchKernelGGL(k_cl_ball_query, dim3(vg_div_up(nq, CL_BQ_WAVES)), dim3(64 * CL_BQ_WAVES), 0, (hipStream_t)stream, d_query, nq,
                       qstride, h->d_spts, h->d_perm, h->grid_n, h->d_grid, h->d_cell_start, r2, reach, nsample, d_idx, d_cnt);
    VG_LAUNCH_CHECK();
    return VG_OK;
}

/* pcdet's loop as written: the targets in row order, the first nsample hits, the padding with the first of them. */
int vg_ball_query_host(const float* targets, int n, int tstride, const float* query, int nq, int qstride, float r2, int nsample,
                       int32_t* idx, int32_t* cnt) {
    if (n < 0 || nq < 0 || tstride < 3 || qstride < 3 || !(r2 > 0.f) || nsample < 1 || nsample > VG_BALL_QUERY_MAX_NSAMPLE) return VG_ERR_ARG;
    if (nq == 0) return VG_OK;
    if (!query || !idx || (n > 0 && !targets)) return VG_ERR_ARG;
    for (int i = 0; i < nq; ++i) {
        const float* q = query + (size_t)i * qstride;
        int32_t* row = idx + (size_t)i * nsample;
        int c = 0;
        for (int k = 0; k < n && c < nsample; ++k) {
            const float* t = targets + (size_t)k * tstride;
            if (!(cl_d2_f32(q[0], q[1], q[2], make_float4(t[0], t[1], t[2], 0.f)) < r2)) continue;
            if (c == 0)
                for (int l = 0; l < nsample; ++l) row[l] = k;
            row[c++] = k;
        }
        if (c == 0)                                           // idx[empty_ball_mask] = 0
            for (int l = 0; l < nsample; ++l) row[l] = 0;
        if (cnt) cnt[i] = c;
    }
    return VG_OK;
}

}  // extern "C"
