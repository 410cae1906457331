// Part of cluster.hip (included in place): K2b, the exact k-NN core distances -- the work list (k_cl_blocks), the two cooperative phases
// (k_cl_core_blk, k_cl_core_far) with the two homes of a lane's list (ClRegList, ClLdsHeap), and their launch path (cl_launch_core).
// Expects cluster_geom.inc, vg_cluster with the ClCounter words, and cl_dbg_counts.

// ---------------------------------------------------------------------------------------------
// Cooperative exact k-NN core distances (north_star: "LDS-staged radius-neighbour / HDBSCAN core-distance kernel over
// Morton-sorted points with coalesced HBM reads").  Two phases, both exact, both bit-identical to the per-point walk they replaced (k_cl_core, dev/cluster_dev.inc: the same
// float64 pair distances; the k-th smallest value does not depend on the order in which the pairs are met):
//   A  k_cl_core_blk   one WAVE per (0.8 m block, 64 queries): the queries of a level-1 node are 64 consecutive sorted points,
//                      lane = query.  The 27 neighbouring level-1 nodes are 27 contiguous ranges of the sorted array: they are
//                      read with coalesced loads (one point per lane), staged in LDS and scanned by every lane (broadcast
//                      reads) into its list of the smallest distances (entered only when some lane improves).  A
//                      neighbour node is skipped when its box is at least as far as every lane's current k-th distance.  A
//                      lane is DONE when its k-th distance does not exceed the distance to the shell's outer faces (nothing
//                      outside the 2.4 m cube can be closer); the others -- isolated points, ~8 % of a LiDAR frame -- go on a
//                      list with their k-th distance so far as an upper bound.
//   B  k_cl_core_far   one WAVE per listed query, lane = candidate: the level-L 3x3x3 shell that covers the bound (L = 2..6) is
//                      expanded to its 27 x 64 level-(L-2) sub-nodes lane-parallel (range + box distance per lane), the
//                      sub-nodes nearer than the running k-th distance are streamed 64 points at a time (coalesced), and the
//                      wave keeps ONE sorted list of the smallest distances across its lanes (lane = rank; insert = a shift
//                      by one lane, max, min).  No per-lane dependent walk: the slowest lane of the old kernel (an isolated
//                      point opening ~100 nodes, each behind two dependent reads of the 64 MB cell table) no longer sets the
//                      launch time.
// Each phase is ONE kernel body.  Only the home of the "k smallest so far" comes in two forms, picked from k by cl_launch_core:
//   k <= 15 (k < CL_K): both lists count the query itself, entry 0 at distance 0, so entry k is the answer.
//     A  ClRegList        the lane's top-16 in registers, inserted by a min / max chain.
//     B  WIDE = false     the sorted list lies in lanes 0..15: the shift by one lane is one row DPP shift (two DPP moves).
//   16 <= k <= VG_CLUSTER_MAX_K (= 64): both lists hold the k nearest OTHER points (entry k - 1 is the answer): the query itself
//   is left out -- in phase B by its index, in phase A, where a staged candidate no longer knows its index, as the first candidate
//   at distance exactly 0 (the query meets itself once, in its own node; a coincident point met first stands in for it with the
//   same value).
//     A  ClLdsHeap<KCAP>  a register min / max chain of 64 float64 does not fit, so each lane keeps a MAX-HEAP of k float64 in
//                         LDS, heap[r * 64 + lane]: whatever rank each lane is at, lane l touches banks 2l and 2l + 1 (mod 64)
//                         of its ds_read_b64 / ds_write_b64 and only lanes 32 apart share them, which are served in different
//                         groups -- conflict-free under any divergence.  The root is the lane's k-th distance (kept in a
//                         register next to the float32 screen); a candidate below it replaces the root and sifts down, at most
//                         log2(k) = 6 levels of two reads and a write.  The k-th smallest VALUE does not depend on the order
//                         of arrival, so the result equals the sorted chain's bit for bit.
//                         LDS per wave (= workgroup): KCAP * 512 B heap + 2.5 .. 3 KB staging.  KCAP = 32 (k <= 32): 19 KB -> 8
//                         waves per CU of the 160 KB; KCAP = 64: 35 KB -> 4 waves per CU (one per SIMD).
//     B  WIDE = true      the sorted list covers all 64 lanes.  An insert is the same shift / max / min; the shift by one lane
//                         is the row DPP shift plus the three values that cross a 16-lane row (lanes 15, 31, 47 -> 16, 32,
//                         48).  64 lanes are what fixes the upper limit of k.
__constant__ signed char CLB_ORDER[27][3] = {
    {0, 0, 0},
    {-1, 0, 0}, {1, 0, 0}, {0, -1, 0}, {0, 1, 0}, {0, 0, -1}, {0, 0, 1},
    {-1, -1, 0}, {1, -1, 0}, {-1, 1, 0}, {1, 1, 0}, {-1, 0, -1}, {1, 0, -1}, {-1, 0, 1}, {1, 0, 1}, {0, -1, -1}, {0, 1, -1}, {0, -1, 1}, {0, 1, 1},
    {-1, -1, -1}, {1, -1, -1}, {-1, 1, -1}, {1, 1, -1}, {-1, -1, 1}, {1, -1, 1}, {-1, 1, 1}, {1, 1, 1}};
#define CLB_TILE 128                  // candidates staged per pass (two coalesced loads per lane)

// (h, v) <- (min(h, v), max(h, v)) for non-NaN doubles
__device__ __forceinline__ void cl_minmax(double& h, double& v) {
    double lo, hi;
    asm("v_min_f64 %0, %1, %2" : "=v"(lo) : "v"(h), "v"(v));
    asm("v_max_f64 %0, %1, %2" : "=v"(hi) : "v"(h), "v"(v));
    h = lo;
    v = hi;
}

// Work list of the cooperative kernels.  A work item = up to 64 consecutive sorted points = the points of ONE octree node,
// chosen top-down from level 3 (3.2 m): a node that holds at most 64 points is one item (lane utilisation: a LiDAR frame's
// 0.8 m nodes hold 9 points on average), a fuller node is split into its children, level-0 cells (0.4 m) are cut into chunks of
// 64.  The item's candidates are the 27 nodes around it AT ITS LEVEL, so sparse regions get a wide shell (more queries end in
// the cooperative phase) and dense surfaces near the sensor a narrow one (a 0.8 m node there holds up to ~600 points with
// ~4 000 in its shell; the heaviest item sets the launch time).  entry = first query index | level << 30.
#define CLB_TOP 1                     // coarsest work-item level (levels 2 / 3 were measured: their shells next to dense objects hold
                                      // 10-20 k candidates and the heaviest item sets the launch time: 832 us instead of 267)
#define CLB_SPLIT 96                  // a level-1 node with more points than this is handled cell by cell
#define CLB_SHELL_CAP 4096            // ... and so is one whose level + 2 ancestor (a 4 x 4 x 4 block that holds most of its shell) is crowded
__global__ void k_cl_blocks(int n, const unsigned int* __restrict__ code_s, const int* __restrict__ cs,
                            unsigned int* __restrict__ entries, int* __restrict__ counters) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned int code = code_s[i], prev = i > 0 ? code_s[i - 1] : ~code;
    if (prev == code) return;                             // not the first point of any node
    // the node that holds point i at every level up to CLB_TOP + 2: its range (independent reads of the cell table)
    int j0[CLB_TOP + 3], j1[CLB_TOP + 3];
#pragma unroll
    for (int lv = 0; lv <= CLB_TOP + 2; ++lv) {
        const unsigned int kk = code >> (3 * lv);
        j0[lv] = cl_start_l(cs, lv, kk);
        j1[lv] = cl_start_l(cs, lv, kk + 1u);
    }
    // a node "fits" when it fills at most one wave and its surroundings are not crowded (the item's cost is its shell's
    // population); the work item of point i's branch is the coarsest node that fits (cells always do, in chunks of 64)
    bool fits[CLB_TOP + 2];
    fits[0] = true;
#pragma unroll
    for (int lv = 1; lv <= CLB_TOP; ++lv) fits[lv] = (j1[lv] - j0[lv]) <= CLB_SPLIT && (j1[lv + 2] - j0[lv + 2]) <= CLB_SHELL_CAP;
    fits[CLB_TOP + 1] = false;
#pragma unroll
    for (int lv = 0; lv <= CLB_TOP; ++lv) {
        if (j0[lv] != i) break;                           // i does not start this node, nor any coarser one
        if (!fits[lv] || fits[lv + 1]) continue;
        const int cnt = j1[lv] - j0[lv];
        const int chunks = (cnt + 63) >> 6;
        const int base = atomicAdd(&counters[CL_CNT_ITEMS], chunks);
        for (int c = 0; c < chunks; ++c) entries[base + c] = (unsigned int)(i + (c << 6)) | ((unsigned int)lv << 30);
    }
}

// Staging plan of one pass of a cooperative kernel: the candidates of up to 27 neighbour nodes, CONCATENATED, so that one
// pass (one round trip to memory for the whole wave) covers a whole neighbourhood when it holds <= CLB_TILE points -- most of
// them do.  seg[t] = {first sorted index, points taken, offset in the tile}; filled by wave-uniform code.
struct ClbPlan {
    int start[27], take[27], off[28];
};
// sorted index of the tile's f-th candidate
__device__ __forceinline__ int clb_locate(const ClbPlan& p, int nseg, int f) {
    int t = 0;
    for (int u = 1; u < nseg; ++u) t += (f >= p.off[u]) ? 1 : 0;
    return p.start[t] + (f - p.off[t]);
}

// The squared distances one lane (= query) of phase A keeps, in the two forms described above.  reset() runs between the two
// barriers in front of an item's first pass.  kth() is the lane's k-th distance so far, worst() the value a candidate has to beat
// to enter at all.  offer() starts with a wave-uniform gate in both forms: nothing happens unless some lane takes the value.
struct ClRegList {
    // ascending; the query meets itself and stays as entry 0.  A vector, not an array: kth() indexes it with the run-time k, and
    // an array inside a struct would leave the registers for scratch memory over that
    typedef double Slots __attribute__((ext_vector_type(CL_K)));
    Slots h;
    __device__ __forceinline__ void chain(int u, double& x) { double e = h[u]; cl_minmax(e, x); h[u] = e; }
    __device__ __forceinline__ void reset(int) {
#pragma unroll
        for (int j = 0; j < CL_K; ++j) h[j] = INFINITY;
    }
    __device__ __forceinline__ double kth(int k) const { return h[k]; }
    __device__ __forceinline__ double worst() const { return h[CL_K - 1]; }      // the last entry whatever k is
    __device__ __forceinline__ void offer(double x, int) {
        if (!__any(x < h[CL_K - 1])) return;
        // sorted insert as a min / max chain.  Raw v_min_f64 / v_max_f64: the operands are squared distances or
        // +inf, never NaN, so the canonicalising v_max_f64 x, x that fmin / fmax put in front of every operand in
        // IEEE mode (half of the chain's instructions) is not needed.  The lower half of the list is entered only
        // when some lane's value belongs there.
        if (__any(x < h[CL_K / 2 - 1])) {
#pragma unroll
            for (int u = 0; u < CL_K / 2; ++u) chain(u, x);
        }
#pragma unroll
        for (int u = CL_K / 2; u < CL_K; ++u) chain(u, x);
    }
};
template <int KCAP>
struct ClLdsHeap {
    double* hp;                                       // this lane's column of the heap
    double top;                                       // the heap's root: the lane's k-th distance so far
    bool self_seen;
    __device__ __forceinline__ void reset(int k) {
        __shared__ double heap[KCAP * 64];            // per-lane max-heap of k entries, lane-interleaved
        hp = heap + threadIdx.x;
        for (int r = 0; r < k; ++r) hp[r * 64] = INFINITY;
        top = INFINITY;
        self_seen = false;
    }
    __device__ __forceinline__ double kth(int) const { return top; }
    __device__ __forceinline__ double worst() const { return top; }
    __device__ __forceinline__ void offer(double x, int k) {
        if (x == 0.0 && !self_seen) { self_seen = true; x = INFINITY; }          // the query itself
        if (!__any(x < top)) return;
        if (x < top) {
            // replace the root by x and sift it down (children of r: 2r + 1, 2r + 2; a missing child reads as -1 < any distance)
            int r = 0;
            for (;;) {
                int c = 2 * r + 1;
                if (c >= k) break;
                double a = hp[c * 64];
                const double b = c + 1 < k ? hp[(c + 1) * 64] : -1.0;
                if (b > a) { a = b; ++c; }
                if (a <= x) break;
                hp[r * 64] = a;
                r = c;
            }
            hp[r * 64] = x;
            top = hp[0];
        }
    }
};

template <int DIM, typename List>
__global__ __launch_bounds__(64) void k_cl_core_blk(const float4* __restrict__ spts, const float* __restrict__ stt, int n,
                                                    const ClGrid* __restrict__ gp, const int* __restrict__ cs,
                                                    const unsigned int* __restrict__ code_s, const unsigned int* __restrict__ entries,
                                                    int* __restrict__ counters, int k, double* __restrict__ core2,
                                                    int* __restrict__ far_list, int* __restrict__ dbg_scan) {
    __shared__ int bnd[27][2];
    __shared__ ClbPlan plan;
    __shared__ float4 tile[CLB_TILE];                 // x, y, z, 4th coordinate
    __shared__ float tile_t[DIM >= 5 ? CLB_TILE : 1]; // 5th coordinate
    const int lane = threadIdx.x;
    const ClGrid g = *gp;
    const int n_entries = counters[CL_CNT_ITEMS];
    for (int e = blockIdx.x; e < n_entries; e += gridDim.x) {
        const int lv = (int)(entries[e] >> 30), i0 = (int)(entries[e] & 0x3FFFFFFFu);   // node level (0 .. 3), first query
        const unsigned int key = code_s[i0] >> (3 * lv);
        const int iend = min(cl_start_l(cs, lv, key + 1u), i0 + 64);
        const int i = i0 + lane;
        const bool active = i < iend;
        const float4 qf = spts[active ? i : i0];
        const float qtf = DIM >= 5 ? stt[active ? i : i0] : 0.f;
        const double qx = qf.x, qy = qf.y, qz = qf.z, qe = qf.w, qt = qtf;
        int bx, by, bz;                                   // the node's coordinates at its level (wave-uniform: from its first point)
        {
            const float4 f0 = spts[i0];
            cl_cell_of(g, (double)f0.x, (double)f0.y, (double)f0.z, bx, by, bz);
            bx >>= lv; by >>= lv; bz >>= lv;
        }
        __syncthreads();                                  // the previous entry's reads of bnd / plan / tile are over
        if (lane < 27) {
            const int nx = bx + CLB_ORDER[lane][0], ny = by + CLB_ORDER[lane][1], nz = bz + CLB_ORDER[lane][2];
            int j0 = 0, j1 = 0;
            if (nx >= 0 && ny >= 0 && nz >= 0 && nx < (CL_NX >> lv) && ny < (CL_NY >> lv) && nz < (CL_NZ >> lv)) {
                const unsigned int c0 = cl_code(nx << lv, ny << lv, nz << lv);
                j0 = cl_start_l(cs, lv, c0 >> (3 * lv));
                j1 = cl_start_l(cs, lv, (c0 >> (3 * lv)) + 1u);
            }
            bnd[lane][0] = j0;
            bnd[lane][1] = j1;
        }
        List list;
        list.reset(k);
        __syncthreads();
        float thr = INFINITY;                             // float32 screen: a candidate whose float32 distance exceeds it cannot enter the list
        int scanned = 0;
        int t_next = 0, cur = bnd[0][0];                  // next neighbour node to plan, next point of it
        while (t_next < 27) {
            // ---- plan one pass (wave-uniform) ----
            int nseg = 0, tot = 0;
            while (t_next < 27 && tot < CLB_TILE) {
                const int j1 = bnd[t_next][1];
                bool need = cur < j1;
                if (need) {
                    // the node's box against every lane's k-th distance so far (same rule as the walk: >= cannot lower it)
                    const double nb2 = cl_box_d2(g, qx, qy, qz, lv, bx + CLB_ORDER[t_next][0], by + CLB_ORDER[t_next][1], bz + CLB_ORDER[t_next][2]);
                    need = __any(active && nb2 < list.kth(k));
                }
                if (need) {
                    const int take = min(j1 - cur, CLB_TILE - tot);
                    if (lane == 0) { plan.start[nseg] = cur; plan.take[nseg] = take; plan.off[nseg] = tot; }
                    ++nseg; tot += take; cur += take;
                    if (cur < j1) break;                  // tile full: the rest of this node in the next pass
                }
                ++t_next;
                if (t_next < 27) cur = bnd[t_next][0];
            }
            if (tot == 0) break;
            __syncthreads();
            // ---- stage: coalesced within each node's range ----
#pragma unroll
            for (int r = 0; r < CLB_TILE / 64; ++r) {
                const int f = lane + 64 * r;
                if (f < tot) {
                    const int j = clb_locate(plan, nseg, f);
                    tile[f] = spts[j];
                    if (DIM >= 5) tile_t[f] = stt[j];
                }
            }
            __syncthreads();
            scanned += tot;
            // ---- scan, four candidates per trip.  Screen in float32 first: the float64 distance of the (exactly converted)
            // float32 coordinates differs from this float32 evaluation by a few ulp, the threshold carries a 1e-5 margin, so
            // a candidate the screen drops is farther than the lane's worst listed distance and the exact list never misses one ----
            for (int c0 = 0; c0 < tot; c0 += 4) {
                float4 p[4];
                float sd[4];
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    p[v] = tile[min(c0 + v, tot - 1)];
                    const float dx = qf.x - p[v].x, dy = qf.y - p[v].y, dz = qf.z - p[v].z;
                    float d = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
                    if (DIM >= 4) { const float de = qf.w - p[v].w; d = fmaf(de, de, d); }
                    if (DIM >= 5) { const float dt = qtf - tile_t[min(c0 + v, tot - 1)]; d = fmaf(dt, dt, d); }
                    sd[v] = c0 + v < tot ? d : INFINITY;
                }
                if (!__any(fminf(fminf(sd[0], sd[1]), fminf(sd[2], sd[3])) <= thr)) continue;
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    if (!__any(sd[v] <= thr)) continue;
                    const double dx = qx - (double)p[v].x, dy = qy - (double)p[v].y, dz = qz - (double)p[v].z;
                    double x = (dx * dx + dy * dy) + dz * dz;
                    if (DIM >= 4) { const double de = qe - (double)p[v].w; x = x + de * de; }
                    if (DIM >= 5) { const double dt = qt - (double)tile_t[min(c0 + v, tot - 1)]; x = x + dt * dt; }
                    if (c0 + v >= tot) x = INFINITY;
                    list.offer(x, k);
                    thr = (float)list.worst() * 1.00001f + 1e-30f;      // unchanged when no lane took x; (float)(+inf) stays +inf
                }
            }
        }
        // nothing outside the 3 x 3 x 3 shell is nearer than its outer faces
        const double r2 = cl_block_radius2(g, qx, qy, qz, bx, by, bz, lv);
        const bool done = list.kth(k) <= r2;
        if (active) {
            core2[i] = list.kth(k);                       // final, or an upper bound for phase B
            if (dbg_scan) dbg_scan[i] = scanned;
        }
        const unsigned long long far = __ballot(active && !done);
        if (far) {
            int base = 0;
            if (lane == 0) base = atomicAdd(&counters[CL_CNT_FAR], __popcll(far));
            base = __shfl(base, 0);
            if (active && !done) far_list[base + __popcll(far & ((1ull << lane) - 1ull))] = i;
        }
    }
}

// value of lane l - 1 within the 16-lane row (0 for the row's first lane): the neighbour a sorted insert needs
__device__ __forceinline__ double cl_row_shr1(double v) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(b & 0xFFFFFFFFll), 0x111, 0xF, 0xF, true);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), 0x111, 0xF, 0xF, true);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
__device__ __forceinline__ double cl_readlane_d(double v, int l) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)(b & 0xFFFFFFFFll), l);
    const int hi = __builtin_amdgcn_readlane((int)(b >> 32), l);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
// value of lane l - 1 across the whole wave (0 for lane 0): the row shift, and lanes 16 / 32 / 48 take the last lane of the row below
__device__ __forceinline__ double cl_wave_shr1(double v, int lane) {
    double p = cl_row_shr1(v);
    const double e15 = cl_readlane_d(v, 15), e31 = cl_readlane_d(v, 31), e47 = cl_readlane_d(v, 47);
    p = lane == 16 ? e15 : p;
    p = lane == 32 ? e31 : p;
    p = lane == 48 ? e47 : p;
    return p;
}

template <int DIM, bool WIDE>
__global__ __launch_bounds__(64) void k_cl_core_far(const float4* __restrict__ spts, const float* __restrict__ stt, int n,
                                                    const ClGrid* __restrict__ gp, const int* __restrict__ cs,
                                                    const int* __restrict__ far_list, const int* __restrict__ counters, int k,
                                                    double* __restrict__ core2, int* __restrict__ dbg_scan) {
    const int lane = threadIdx.x;
    const ClGrid g = *gp;
    const int n_far = counters[CL_CNT_FAR];
    for (int u = blockIdx.x; u < n_far; u += gridDim.x) {
        const int i = far_list[u];
        const float4 qf = spts[i];
        const double qx = qf.x, qy = qf.y, qz = qf.z, qe = qf.w, qt = DIM >= 5 ? (double)stt[i] : 0.0;
        int cx, cy, cz;
        cl_cell_of(g, qx, qy, qz, cx, cy, cz);
        const double bound = core2[i];                    // phase A's k-th distance: the true one is not larger
        int L = 2;
        while (L < CL_LMAX && !(bound <= cl_block_radius2(g, qx, qy, qz, cx >> L, cy >> L, cz >> L, L))) ++L;
        if (isinf(bound)) L = 3;
        const int kl = WIDE ? k - 1 : k;                  // the lane that holds the answer
        double hs = g.inf;                                // lane r: the r-th smallest distance so far (WIDE: the (r + 1)-th to another point)
        double T = g.inf;                                 // = lane kl's entry (wave-uniform; see ClGrid::inf)
        int scanned = 0;
        for (;;) {
            hs = g.inf; T = g.inf;
            auto stream = [&](int j0, int j1) {
                for (int base = j0; base < j1; base += 64) {
                    const int j = base + lane;
                    double d2 = INFINITY;
                    if (j < j1 && (!WIDE || j != i)) d2 = cl_d2<DIM>(qx, qy, qz, qe, qt, spts[j], stt, j);
                    scanned += min(64, j1 - base);
                    unsigned long long pm = __ballot(d2 < T);
                    while (pm) {
                        const int b = __ffsll((long long)pm) - 1;
                        pm &= pm - 1;
                        const double v = cl_readlane_d(d2, b);
                        if (v < T) {
                            double mx, prev = WIDE ? cl_wave_shr1(hs, lane) : cl_row_shr1(hs);
                            asm("v_max_f64 %0, %1, %2" : "=v"(mx) : "v"(prev), "v"(v));
                            asm("v_min_f64 %0, %1, %2" : "=v"(hs) : "v"(mx), "v"(hs));
                            T = cl_readlane_d(hs, kl);
                        }
                    }
                }
            };
            if (L > CL_LMAX) {                            // the grid's roots did not settle it: every point (exact for any input)
                stream(0, n);
                break;
            }
            const int BX = cx >> L, BY = cy >> L, BZ = cz >> L;
            const int l2 = L - 2;
            for (int t = 0; t < 27; ++t) {
                const int nx = BX + CLB_ORDER[t][0], ny = BY + CLB_ORDER[t][1], nz = BZ + CLB_ORDER[t][2];
                if (nx < 0 || ny < 0 || nz < 0 || nx >= (CL_NX >> L) || ny >= (CL_NY >> L) || nz >= (CL_NZ >> L)) continue;
                if (cl_box_d2(g, qx, qy, qz, L, nx, ny, nz) >= T) continue;
                // the node's 64 level-(L-2) sub-nodes, one per lane (Morton order: consecutive ranges)
                const unsigned int c0 = cl_code(nx << L, ny << L, nz << L);
                const int s0 = cl_start_l(cs, l2, (c0 >> (3 * l2)) + (unsigned int)lane);
                const int s1 = cl_start_l(cs, l2, (c0 >> (3 * l2)) + (unsigned int)lane + 1u);
                const int sx = (nx << 2) | (((lane >> 3) & 1) << 1) | (lane & 1);
                const int sy = (ny << 2) | (((lane >> 4) & 1) << 1) | ((lane >> 1) & 1);
                const int sz = (nz << 2) | (((lane >> 5) & 1) << 1) | ((lane >> 2) & 1);
                const double sb2 = cl_box_d2(g, qx, qy, qz, l2, sx, sy, sz);
                unsigned long long sm = __ballot(s0 != s1 && sb2 < T);
                while (sm) {
                    const int b = __ffsll((long long)sm) - 1;
                    sm &= sm - 1;
                    if (cl_readlane_d(sb2, b) >= T) continue;
                    stream(__builtin_amdgcn_readlane(s0, b), __builtin_amdgcn_readlane(s1, b));
                }
            }
            if (T <= cl_block_radius2(g, qx, qy, qz, BX, BY, BZ, L)) break;
            ++L;
        }
        if (lane == 0) {
            core2[i] = T;
            if (dbg_scan) dbg_scan[i] += scanned;
        }
    }
}

// the two cooperative phases in one form (List / WIDE: see k_cl_core_blk)
template <int DIM, typename List, bool WIDE>
static void cl_launch_core_phases(vg_cluster* h, int n, int k, hipStream_t st) {
    hipLaunchKernelGGL((k_cl_core_blk<DIM, List>), dim3(std::min(n, 16384)), dim3(64), 0, st, h->d_spts, h->d_st, n, h->d_grid, h->d_cell_start,
                       h->d_code_s, h->d_entries, h->d_counter, k, h->d_core2, h->d_far, h->d_dbg);
    hipLaunchKernelGGL((k_cl_core_far<DIM, WIDE>), dim3(std::min(n, 8192)), dim3(64), 0, st, h->d_spts, h->d_st, n, h->d_grid, h->d_cell_start,
                       h->d_far, h->d_counter, k, h->d_core2, h->d_dbg);
}

#ifdef VG_DEV      // dev/cluster_dev.inc, included by cluster_mst.inc behind the walk's launch it also needs
template <int DIM>
static bool cl_dev_core_walk(vg_cluster* h, int n, int k, hipStream_t st);
#endif
template <int DIM>
static void cl_launch_core(vg_cluster* h, int n, int k, hipStream_t st) {
    bool walked = false;                              // (the per-point walk ran instead: no work list, no far phase)
#ifdef VG_DEV
    walked = cl_dev_core_walk<DIM>(h, n, k, st);
#endif
    if (!walked) {
        // the work-list entries of phase A and the queries left for phase B: two adjacent words (see ClCounter)
        (void)hipMemsetAsync(h->d_counter + CL_CNT_ITEMS, 0, (CL_CNT_FAR + 1 - CL_CNT_ITEMS) * sizeof(int), st);
        hipLaunchKernelGGL(k_cl_blocks, dim3(vg_div_up(n, 256)), dim3(256), 0, st, n, h->d_code_s, h->d_cell_start, h->d_entries, h->d_counter);
        if (k < CL_K) cl_launch_core_phases<DIM, ClRegList, false>(h, n, k, st);
        else if (k <= 32) cl_launch_core_phases<DIM, ClLdsHeap<32>, true>(h, n, k, st);
        else cl_launch_core_phases<DIM, ClLdsHeap<64>, true>(h, n, k, st);
    }
    if (h->d_dbg) {
        // VG_CLUSTER_DEBUG=1: pairs evaluated / pairs needed (SURVEY 8d): the exact answer needs n * k distances
        const ClDbgCounts sc = cl_dbg_counts(h, n, st);
        int cnt[CL_CNT_FAR + 1] = {0};
        (void)hipMemcpy(cnt, h->d_counter, sizeof(cnt), hipMemcpyDeviceToHost);
        fprintf(stderr, "[cluster dbg] core distances: n %d, k %d, pair distances evaluated %lld = %.1f x the %lld needed (n*k); per point median %d, p99 %d, max %d"
                        "; cooperative: %d (node, 64-query) work items, %d queries left to the far phase\n",
                n, k, sc.total, (double)sc.total / ((double)n * k), (long long)n * k, sc.at(1, 2), sc.at(99, 100), sc.max(), walked ? 0 : cnt[CL_CNT_ITEMS], walked ? 0 : cnt[CL_CNT_FAR]);
    }
}
