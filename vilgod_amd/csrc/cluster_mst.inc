// Part of cluster.hip (included in place): K2c, the Boruvka minimum spanning tree of the mutual-reachability graph -- the kernels of a
// round (k_cl_b_*), the edge sort's helpers, the MST's switches and the walk's launch, the development build's include, and cl_mst.
// Expects cluster_geom.inc, cluster_grid.inc (cl_build_grid, cl_e_gap2), cluster_core.inc (cl_launch_core) and the ClCounter words.

// Consecutive hardware workgroup ids are dealt round-robin to the 8 XCDs (observed placement, speed only): logical block = a contiguous run
// of the Morton order per XCD, so that the table lines and points a region's queries share are served by ONE L2 instead of eight
// (round 5: Sigma k_cl_b_search 2 354 -> 2 280 us per MST, two interleaved pairs of traces).
__device__ __forceinline__ int cl_xcd_block(int bid, int nwg) {
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, s = bid >> 3;
    const int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + s;
}

// ---------------------------------------------------------------------------------------------
// Boruvka
#define CL_CYCLE 0x40000000            // bit of the edge counter: k_cl_b_compress found a cycle among the round's picks
#define CL_NONE 0xFFFFFFFFFFFFFFFFull   // 'no candidate' (sorts after every weight, +inf included)

__global__ void k_cl_b_init(int n, int* __restrict__ comp, int* __restrict__ counter, int* __restrict__ pt_b,
                            double* __restrict__ pt_lb, const double* __restrict__ core2, const float* __restrict__ stt,
                            int4* __restrict__ aux, int* __restrict__ csize, unsigned long long* __restrict__ giant) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) *giant = 0ull;
    if (i < n) {
        comp[i] = i; pt_b[i] = -1; pt_lb[i] = 0.0; csize[i] = 1;
        const long long cb = __double_as_longlong(core2[i]);
        aux[i] = make_int4((int)(cb & 0xFFFFFFFFll), (int)(cb >> 32), i, stt ? __float_as_int(stt[i]) : 0);
    }
    if (i == 0) counter[CL_CNT_DONE] = 0;
    if (i == 0) counter[CL_CNT_EDGES] = 0;
}

// A point's candidate of the previous round stays its minimum foreign edge as long as the other end is still foreign
// (components only grow): keep it, and publish its weight as the component's bound BEFORE the searches start, so the
// points that do have to search again (their candidate was absorbed) prune against a tight bound from the first node on.
// Without this every late round -- few, large components -- started all its traversals unbounded (3-4 ms per round).
__global__ void k_cl_b_seed(int n, const int* __restrict__ comp, int* __restrict__ pt_b,
                            const unsigned long long* __restrict__ pt_w, unsigned long long* __restrict__ best_w, const int* __restrict__ flags) {
    if (flags[CL_CNT_DONE]) return;                 // the tree was complete before this round: queued ahead without a host read
    int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= n) return;
    const int b = pt_b[a];
    if (b < 0) return;
    const int c = comp[a];
    if (comp[b] == c) pt_b[a] = -1;                 // absorbed: search again
    else atomicMin(&best_w[c], pt_w[a]);
}

// THE LARGEST COMPONENT DOES NOT SEARCH (round 5).  Boruvka needs, per round, the minimum edge leaving a component only from the components
// that are going to merge along it; any subset of the components may sit a round out -- every edge the others pick is still the minimum
// edge leaving its component, hence an edge of the (unique, strict order) MST, and as long as one other component exists the round makes
// progress.  The component that sits out is the largest one (if it holds at least n / 8 points): in the late rounds it owns most of the
// frame's points, its nearest foreign structure is metres away, and its boundary points were the longest walks of the launch -- while the
// edge that joins it to a neighbour is found from the neighbour's side anyway.  Sizes live at the roots (k_cl_b_init: 1; k_cl_b_compress adds
// an absorbed root's size to its new root); the maximum over the roots is taken here, one atomic per workgroup.
__global__ void k_cl_b_round_init(int n, const int* __restrict__ comp, unsigned long long* __restrict__ best_w,
                                  unsigned long long* __restrict__ best_d, unsigned long long* __restrict__ best_e,
                                  int* __restrict__ sel_a, const int* __restrict__ flags, const int* __restrict__ csize,
                                  unsigned long long* __restrict__ giant, const unsigned int* __restrict__ code_s,
                                  int* __restrict__ cell_comp) {
    if (flags[CL_CNT_DONE]) return;                 // the tree was complete before this round: queued ahead without a host read
    __shared__ unsigned long long blk_max[4];
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long mine = 0ull;
    if (i < n) {
        best_w[i] = CL_NONE;
        best_d[i] = ~0ull;
        best_e[i] = ~0ull;
        sel_a[i] = -1;
        if (comp[i] == i) mine = ((unsigned long long)(unsigned int)csize[i] << 32) | (unsigned int)i;
        // purity tables, first half: the first point of every node of levels 0 .. 3 writes its component; k_cl_b_purity (a later launch)
        // overwrites the entry with -1 where two neighbours inside the node disagree
        {
            const unsigned int code = code_s[i], prev = i > 0 ? code_s[i - 1] : ~code;
            size_t off = 0;
#pragma unroll
            for (int l = 0; l < CL_PUR_LEVELS; ++l) {
                if (i == 0 || (prev >> (3 * l)) != (code >> (3 * l))) cell_comp[off + (code >> (3 * l))] = comp[i];
                off += (size_t)CL_NCODES >> (3 * l);
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(mine, o);
        mine = other > mine ? other : mine;
    }
    if ((threadIdx.x & 63) == 0) blk_max[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long m = blk_max[0];
        for (int w = 1; w < (int)(blockDim.x >> 6); ++w) m = blk_max[w] > m ? blk_max[w] : m;
        if (m) atomicMax(giant, m);
    }
}
// does component c sit this round out?
__device__ __forceinline__ bool cl_sits_out(unsigned long long giant, int c, int min_size) {
    return (int)(giant >> 32) >= min_size && (int)(giant & 0xFFFFFFFFull) == c;
}

__device__ __forceinline__ size_t cl_pur_off(int l) {   // offset of level l inside the purity tables
    size_t o = 0;
    for (int i = 0; i < l; ++i) o += (size_t)CL_NCODES >> (3 * i);
    return o;
}

// Purity tables, levels 0 .. 3: entry = the component that owns every point of the node, or -1.  All points of a node agree iff every two
// neighbours in the sorted order agree: k_cl_b_round_init wrote the first point's component at every level, a thread whose point differs
// from its predecessor writes -1 at every level at which the two share a node (same value from every writer).  (Rounds 1-4: the first point
// of a cell walked the whole cell -- 29.5 us per launch, 80 at worst -- and three more launches built levels 1 .. 3 from the level below:
// 0.33 ms and 28 launches per frame; now one compare per thread and one launch per round.)
__global__ void k_cl_b_purity(int n, const unsigned int* __restrict__ code_s, const int* __restrict__ comp,
                              int* __restrict__ cell_comp, const int* __restrict__ flags) {
    if (flags[CL_CNT_DONE]) return;                 // the tree was complete before this round: queued ahead without a host read
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || i == 0) return;
    if (comp[i - 1] == comp[i]) return;
    const unsigned int c = code_s[i], p = code_s[i - 1];
    size_t off = 0;
#pragma unroll
    for (int l = 0; l < CL_PUR_LEVELS; ++l) {
        if ((p >> (3 * l)) == (c >> (3 * l))) cell_comp[off + (c >> (3 * l))] = -1;
        off += (size_t)CL_NCODES >> (3 * l);
    }
}

__device__ __forceinline__ unsigned long long cl_edge_key(int oa, int ob) {
    unsigned int lo = oa < ob ? oa : ob, hi = oa < ob ? ob : oa;
    return ((unsigned long long)lo << 32) | hi;
}

// NT: threads per workgroup.  The walk is bound by its longest dependent chain, not by a CU's resources, and its workgroup's size decides
// how many CUs a launch OCCUPIES: a CU that holds any wave of this kernel cannot take a projection-GEMM tile of another frame's ViT pass
// (that workgroup needs all 160 KB of LDS and every vector register), and the dispatcher deals workgroups round-robin over the CUs:
// 309 workgroups of 256 threads sit on all 256 CUs for the launch's ~300 us, 155 of 512 threads on 155 (two waves per SIMD either way:
// 172 registers, 88 KB of stack per CU).
// Measured and dropped (round 5): leaf CHILDREN scanned from their parent's visit.  A walk is a chain of dependent round trips -- one per
// internal node, two per leaf (its own range, then its points) -- and the parent's trip already brings every child's range and purity, so
// in near-to-far order the leaf children in front of the first internal child were scanned right there: the same visits in the same order,
// one round trip less each.  Bit-identical, and SLOWER: Sigma search 2 290 -> 2 610 us per MST (211 instead of 172 registers; what counts is
// the WAVE's chain: before, all lanes that sat at a leaf in one loop iteration shared its round trip; now a lane scanning five leaf children
// inside one iteration keeps the other 63 lanes waiting five trips).
// Measured and dropped (round 5), second attempt at the same chain: a leaf's points requested ONE ITERATION LATE, beside the next node's tables
// (a "pending" range per lane; stale bounds prune less, never wrongly): one round trip per iteration instead of two, bit-identical, 187
// registers -- and 8 % slower (Sigma search 2 330 -> 2 520 us, two interleaved pairs of traces).  Together with the first attempt this says
// the walk is NOT bound by its memory round trips: with ~1.2 waves per SIMD a wave pays for the INSTRUCTIONS of every path some lane takes
// in an iteration (float64 box tests of eight children, the sixteen-point screen + exact chain), and both variants added instructions.
// Measured and dropped (round 4): rounds >= 2 over a compacted list of the points that still have to walk (a few thousand; one 6 us
// launch builds it): bit-identical, and the rounds take as long as before (332 vs 316 us: a round lasts as long as its longest walks,
// however few waves carry them) while the pipeline's frames/s do not move (65.1 vs 65.2) -- the walks do not keep GEMM tiles waiting.
template <int DIM, int NT>
__global__ __launch_bounds__(NT) void k_cl_b_search(const float4* __restrict__ spts, const float* __restrict__ stt, int n,
                                                     const ClGrid* __restrict__ gp, const int* __restrict__ cs,
                                                     const int* __restrict__ cell_comp, const unsigned int* __restrict__ cell_e,
                                                     const int* __restrict__ perm,
                                                     const double* __restrict__ core2, const int* __restrict__ comp,
                                                     const int4* __restrict__ aux,
                                                     unsigned long long* __restrict__ best_w,
                                                     unsigned long long* __restrict__ pt_w,
                                                     unsigned long long* __restrict__ pt_d,
                                                     unsigned long long* __restrict__ pt_key, int* __restrict__ pt_b,
                                                     double* __restrict__ pt_lb, int* __restrict__ dbg_scan, const int* __restrict__ flags,
                                                     const unsigned long long* __restrict__ giant, int sit_min, int xcd_order) {
    if (flags[CL_CNT_DONE]) return;                 // the tree was complete before this round: queued ahead without a host read
    __shared__ unsigned int stack[CL_STACK * NT];
    int a = (xcd_order ? cl_xcd_block(blockIdx.x, gridDim.x) : (int)blockIdx.x) * blockDim.x + threadIdx.x;
    if (a >= n) return;
    int scanned = 0;
    if (dbg_scan) dbg_scan[a] = 0;
    unsigned int* st = stack + threadIdx.x;
    const ClGrid g = *gp;
    const float4 qf = spts[a];
    const float qtf = DIM >= 5 ? stt[a] : 0.f;
    const double qx = qf.x, qy = qf.y, qz = qf.z, qe = qf.w, qt = qtf;
    if (pt_b[a] >= 0) return;                        // candidate of an earlier round still valid (k_cl_b_seed)
    const int ca = comp[a];
    if (cl_sits_out(*giant, ca, sit_min)) {          // the largest component does not search this round (k_cl_b_round_init)
        pt_w[a] = CL_NONE; pt_d[a] = ~0ull; pt_key[a] = ~0ull; pt_b[a] = -1;
        return;
    }
    const double core_a = core2[a];
    // Every edge that leaves a's component from a weighs at least lb_a: its mutual-reachability weight is >= core_a, and
    // >= the bound carried over from earlier rounds (a's own minimum foreign edge then, or the winning weight of its
    // component when a was pruned) -- the foreign set only shrinks.  A point whose bound already exceeds the component's
    // published best cannot supply the component's edge: interior points of large components drop out at once.
    const double lb_a = fmax(core_a, pt_lb[a]);
    {
        const unsigned long long cb0 = __hip_atomic_load(&best_w[ca], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cb0 != CL_NONE && lb_a > __longlong_as_double((long long)cb0)) {
            pt_w[a] = CL_NONE; pt_d[a] = ~0ull; pt_key[a] = ~0ull; pt_b[a] = -1;
            return;
        }
    }
    const int oa = perm[a];
    int cx, cy, cz;
    cl_cell_of(g, qx, qy, qz, cx, cy, cz);
    // edges are ordered by (w, d2, original ids): mutual-reachability weight, then the pair's own squared distance.
    // w = core_a for EVERY neighbour inside a's core ball whose core distance is not larger, so ties on w are the
    // rule; breaking them by d2 lets the traversal stop at the nearest such neighbour (nodes farther than bd2 cannot
    // win a tie) instead of scanning the whole ball for the smallest id.
    double bw = INFINITY;          // best weight found by this point
    double bd2 = INFINITY;         // ... and that edge's squared pair distance
    double cbest = INFINITY;       // best weight published for the whole component (read again now and then)
    int since_refresh = 64;        // ... first with the first node
    unsigned long long bkey = ~0ull;   // ... and its id key -- computed only when an exact (w, d2) tie asks for it, and at the end
    bool bkey_valid = true;
    int bb = -1;
    // The slowest WAVE sets the launch time (1 234 waves on 1 024 SIMDs: nothing else hides a wave's stalls), and a wave pays for
    // whatever any of its lanes does (per-thread stamps, round 3: the median wave of round 1 runs 180 us in which its slowest
    // lane waits 6 us for node reads and spends 15-45 us in leaf scans -- the rest is other lanes' scans).  Hence:
    //  * a node costs ONE memory round trip: the ranges of its eight children (nine consecutive entries of the level below: they
    //    include the node's own range), its purity entry, its 4th-coordinate range and -- every 8th node and after a leaf scan --
    //    the component's published bound are requested together;
    //  * a leaf scan loads sixteen points per trip, each as two 16-byte records (coordinates; core distance, component, 5th
    //    coordinate): no second trip for the survivors' core distances, none for ids (read only on an exact tie);
    //  * a point of the own component, or farther than the best edge so far, is dropped by a float32 screen.
    const int rx0 = cx >> CL_LMAX, ry0 = cy >> CL_LMAX;
    const int nrx = CL_NX >> CL_LMAX, nry = CL_NY >> CL_LMAX;
    for (int rr = 0; rr < nrx * nry; ++rr) {
        int rx = rr % nrx, ry = rr / nrx;
        if (rr == 0) { rx = rx0; ry = ry0; }
        else if (rx == rx0 && ry == ry0) { rx = 0; ry = 0; }
        int sp = 0;
        st[0] = cl_pack(CL_LMAX, rx, ry, 0);
        sp = 1;
        while (sp > 0) {
            int l, x, y, z;
            cl_unpack(st[(--sp) * NT], l, x, y, z);
            // every edge into this node weighs at least lb; it must be able to tie or beat both bounds (ALU only)
            const double nd2 = cl_box_d2(g, qx, qy, qz, l, x, y, z);
            const double lb = fmax(lb_a, nd2);
            if (lb > bw || lb > cbest || (lb == bw && nd2 > bd2)) continue;
            const unsigned int c = cl_code(x << l, y << l, z << l) >> (3 * l);      // the node's number at its level
            // ---- the node's reads, all in flight together ----
            int bnd[9];
            {
                // children ranges: level l - 1, entries 8c .. 8c + 8 (cells: the reversed table); a cell reads its own two ends
                const long long base = l == 0 ? (long long)CL_NCODES - c
                                     : l == 1 ? (long long)CL_NCODES - 8ll * c
                                              : (long long)(CL_NCODES + 1) + (long long)cl_lvl_off(l - 1) + 8ll * c;
                const long long dir = l <= 1 ? -1 : 1;
#pragma unroll
                for (int u = 0; u < 9; ++u) {
                    long long at = base + dir * u;
                    bnd[u] = cs[at < 0 ? 0 : at];
                }
            }
            const bool has_pur = l < CL_PUR_LEVELS;
            const size_t po = has_pur ? cl_pur_off(l) + c : 0;
            const int pure = cell_comp[po];
            const unsigned int erange = DIM >= 4 ? cell_e[po] : 0u;
            // (the bound: in a late round a whole frame's threads belong to two or three components, and a read per node queues up
            // behind the atomics on those few words)
            const bool refresh = ++since_refresh >= 8;
            unsigned long long cb = 0;
            if (refresh) { cb = __hip_atomic_load(&best_w[ca], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); since_refresh = 0; }
            // ---- use them ----
            const int j0 = bnd[0], j1 = l == 0 ? bnd[1] : bnd[8];
            if (refresh) cbest = cb == CL_NONE ? INFINITY : __longlong_as_double((long long)cb);
            if (lb_a > cbest) { sp = 0; rr = nrx * nry; break; }      // this point can no longer win: stop
            if (j0 == j1) continue;
            if (has_pur && pure == ca) continue;         // all ours
            if (DIM >= 4 && has_pur) {
                const double ed2 = nd2 + cl_e_gap2(erange, qe);
                const double elb = fmax(lb_a, ed2);
                if (elb > bw || elb > cbest || (elb == bw && ed2 > bd2)) continue;
            }
            if (l == 0 || j1 - j0 <= CL_LEAF) {
                bool improved = false;
                scanned += j1 - j0;
                // the float64 distance of the (exactly converted) float32 coordinates differs from the float32 evaluation by a few
                // ulp, the threshold carries a 1e-5 margin: a point the screen drops has d2 > bw and could neither win nor tie
                float thr = (float)bw * 1.00001f + 1e-30f;               // (float)(+inf) stays +inf
                for (int jb = j0; jb < j1; jb += 16) {
                    float4 pj[16];
                    int4 xj[16];
#pragma unroll
                    for (int u = 0; u < 16; ++u) {
                        const int j = jb + u < j1 ? jb + u : j1 - 1;
                        pj[u] = spts[j];
                        xj[u] = aux[j];
                    }
#pragma unroll
                    for (int u = 0; u < 16; ++u) {
                        const float fx = qf.x - pj[u].x, fy = qf.y - pj[u].y, fz = qf.z - pj[u].z;
                        float sd = fmaf(fz, fz, fmaf(fy, fy, fx * fx));
                        if (DIM >= 4) { const float fe = qf.w - pj[u].w; sd = fmaf(fe, fe, sd); }
                        if (DIM >= 5) { const float ft = qtf - __int_as_float(xj[u].w); sd = fmaf(ft, ft, sd); }
                        if (!(sd <= thr) || xj[u].z == ca || jb + u >= j1) continue;
                        // (the survivors update the best edge by selects: inside this branch every further branch is paid by the
                        // whole wave; only an exact (w, d2) tie -- rare -- goes on to compare ids)
                        const int j = jb + u;
                        const double dx = qx - (double)pj[u].x, dy = qy - (double)pj[u].y, dz = qz - (double)pj[u].z;
                        double d2 = (dx * dx + dy * dy) + dz * dz;
                        if (DIM >= 4) { const double de = qe - (double)pj[u].w; d2 = d2 + de * de; }
                        if (DIM >= 5) { const double dt = qt - (double)__int_as_float(xj[u].w); d2 = d2 + dt * dt; }
                        const double cj2 = __longlong_as_double(((long long)xj[u].y << 32) | (unsigned int)xj[u].x);
                        const double w = fmax(fmax(d2, core_a), cj2);
                        const bool better = w < bw || (w == bw && d2 < bd2);
                        if (w == bw && d2 == bd2) {      // same weight, same pair distance: the smaller id pair
                            if (!bkey_valid) { bkey = cl_edge_key(oa, perm[bb]); bkey_valid = true; }
                            const unsigned long long key = cl_edge_key(oa, perm[j]);
                            if (key < bkey) { bkey = key; bb = j; }
                        }
                        bw = better ? w : bw;
                        bd2 = better ? d2 : bd2;
                        bb = better ? j : bb;
                        bkey_valid = bkey_valid && !better;
                        improved = improved || better;
                        thr = (float)bw * 1.00001f + 1e-30f;
                    }
                }
                if (improved) atomicMin(&best_w[ca], (unsigned long long)__double_as_longlong(bw));
                since_refresh = 64;
                continue;
            }
            // ---- children: nearest one pushed last.  Sibling boxes share their faces: two distances per axis serve all eight; the
            // push is a store + a conditional count (no branch per child) ----
            const int l1 = l - 1;
            const int ox = ((cx >> l1) > 2 * x) ? 1 : 0, oy = ((cy >> l1) > 2 * y) ? 1 : 0, oz = ((cz >> l1) > 2 * z) ? 1 : 0;
            const int near = ox | (oy << 1) | (oz << 2);
            double ad[3][2];
            {
                const int nbx[3] = {CL_NX >> l1, CL_NY >> l1, CL_NZ >> l1};
                const int c2[3] = {2 * x, 2 * y, 2 * z};
                const double q3[3] = {qx, qy, qz}, o3[3] = {g.ox, g.oy, g.oz};
#pragma unroll
                for (int ax = 0; ax < 3; ++ax)
#pragma unroll
                    for (int hb = 0; hb < 2; ++hb) ad[ax][hb] = cl_axis_gap(o3[ax], q3[ax], c2[ax] + hb, l1, nbx[ax]);
            }
            // child u of the near-first order is octant u ^ near: its range [bnd[u ^ near], bnd[(u ^ near) + 1]) comes out of three conditional
            // exchange stages over the two boundary arrays (48 selects) instead of a 7-deep select chain per child and end (112), and the
            // squared axis distances are taken once per axis half (round 5: the walk is bound by its instruction count)
            int blo[8], bhi[8];
#pragma unroll
            for (int v = 0; v < 8; ++v) { blo[v] = bnd[v]; bhi[v] = bnd[v + 1]; }
#pragma unroll
            for (int bit = 0; bit < 3; ++bit) {
                const bool sw = (near >> bit) & 1;
#pragma unroll
                for (int v = 0; v < 8; ++v)
                    if (!((v >> bit) & 1)) {
                        const int w_ = v | (1 << bit);
                        const int a0 = blo[v], a1 = blo[w_], h0 = bhi[v], h1 = bhi[w_];
                        blo[v] = sw ? a1 : a0; blo[w_] = sw ? a0 : a1;
                        bhi[v] = sw ? h1 : h0; bhi[w_] = sw ? h0 : h1;
                    }
            }
            // (after the exchanges position u holds octant u ^ near; the same for the axis distances: index 0 = the near half)
            const double ax0 = ox ? ad[0][1] : ad[0][0], ax1 = ox ? ad[0][0] : ad[0][1];
            const double ay0 = oy ? ad[1][1] : ad[1][0], ay1 = oy ? ad[1][0] : ad[1][1];
            const double az0 = oz ? ad[2][1] : ad[2][0], az1 = oz ? ad[2][0] : ad[2][1];
            const double sx[2] = {ax0 * ax0, ax1 * ax1}, sy[2] = {ay0 * ay0, ay1 * ay1}, sz[2] = {az0 * az0, az1 * az1};
#pragma unroll
            for (int u = 7; u >= 0; --u) {
                const int ch = u ^ near;
                const int hx = ch & 1, hy = (ch >> 1) & 1, hz = (ch >> 2) & 1;
                double cd2 = 0.0;
                cd2 += sx[u & 1];
                cd2 += sy[(u >> 1) & 1];
                cd2 += sz[(u >> 2) & 1];
                const double clb = fmax(lb_a, cd2);
                const int lo_i = blo[u], hi_i = bhi[u];
                const bool keep = lo_i != hi_i && !(clb > bw || clb > cbest || (clb == bw && cd2 > bd2)) && sp < CL_STACK;
                st[sp * NT] = cl_pack(l1, 2 * x + hx, 2 * y + hy, 2 * z + hz);      // (slot sp is free: written, kept only if counted)
                sp += keep ? 1 : 0;
            }
        }
    }
    if (bb >= 0 && !bkey_valid) bkey = cl_edge_key(oa, perm[bb]);
    if (dbg_scan) dbg_scan[a] = scanned;
    if (bb >= 0 && bw <= cbest) {
        pt_w[a] = (unsigned long long)__double_as_longlong(bw);
        pt_d[a] = (unsigned long long)__double_as_longlong(bd2);
        pt_key[a] = bkey;
        pt_b[a] = bb;
        pt_lb[a] = bw;                       // a's true minimum foreign edge: a lower bound from now on
    } else {
        if (cbest < INFINITY && cbest > pt_lb[a]) pt_lb[a] = cbest;      // everything a left unexplored weighs more than this
        pt_w[a] = CL_NONE;
        pt_d[a] = ~0ull;
        pt_key[a] = ~0ull;
        pt_b[a] = -1;
    }
}

// per component: smallest w (atomicMin in the search), then smallest d2 among those, then smallest id key among those
__global__ void k_cl_b_select_d(int n, const int* __restrict__ comp, const unsigned long long* __restrict__ best_w,
                                const unsigned long long* __restrict__ pt_w, const unsigned long long* __restrict__ pt_d,
                                unsigned long long* __restrict__ best_d, const int* __restrict__ flags) {
    if (flags[CL_CNT_DONE]) return;                 // the tree was complete before this round: queued ahead without a host read
    int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= n) return;
    const int c = comp[a];
    if (pt_w[a] != CL_NONE && pt_w[a] == best_w[c]) atomicMin(&best_d[c], pt_d[a]);
}
__global__ void k_cl_b_select(int n, const int* __restrict__ comp, const unsigned long long* __restrict__ best_w,
                              const unsigned long long* __restrict__ best_d, const unsigned long long* __restrict__ pt_w,
                              const unsigned long long* __restrict__ pt_d, const unsigned long long* __restrict__ pt_key,
                              unsigned long long* __restrict__ best_e, const int* __restrict__ flags) {
    if (flags[CL_CNT_DONE]) return;                 // the tree was complete before this round: queued ahead without a host read
    int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= n) return;
    const int c = comp[a];
    if (pt_w[a] != CL_NONE && pt_w[a] == best_w[c] && pt_d[a] == best_d[c]) atomicMin(&best_e[c], pt_key[a]);
}
__global__ void k_cl_b_pick(int n, const int* __restrict__ comp, const unsigned long long* __restrict__ best_w,
                            const unsigned long long* __restrict__ best_d, const unsigned long long* __restrict__ best_e,
                            const unsigned long long* __restrict__ pt_w, const unsigned long long* __restrict__ pt_d,
                            const unsigned long long* __restrict__ pt_key, const int* __restrict__ pt_b,
                            int* __restrict__ sel_a, int* __restrict__ sel_b, const int* __restrict__ flags,
                            const unsigned long long* __restrict__ giant, int sit_min) {
    if (flags[CL_CNT_DONE]) return;                 // the tree was complete before this round: queued ahead without a host read
    int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= n) return;
    const int c = comp[a];
    // (the component that sits out picks nothing: some of its points still hold candidates of earlier rounds, valid edges but not
    // necessarily the component's minimum since the others did not search)
    if (cl_sits_out(*giant, c, sit_min)) return;
    if (pt_w[a] != CL_NONE && pt_w[a] == best_w[c] && pt_d[a] == best_d[c] && pt_key[a] == best_e[c]) {
        sel_a[c] = a;
        sel_b[c] = pt_b[a];
    }
}
// Every component root c with a pick hooks onto the component its edge leads to: parent(c) = comp[sel_b[c]] (c itself without a pick).  The
// two roots of a mutual pair chose the same edge: the smaller id becomes the root, its partner emits the edge.  (Until round 5 the parents were
// written by a launch of their own, k_cl_b_link; they are a function of the picks, which are complete when this kernel starts.)
__global__ void k_cl_b_emit(int n, const int* __restrict__ comp, const int* __restrict__ sel_a, const int* __restrict__ sel_b,
                            const unsigned long long* __restrict__ best_w, const int* __restrict__ perm,
                            int* __restrict__ parent2, int* __restrict__ counter, int* __restrict__ mst_a,
                            int* __restrict__ mst_b, unsigned long long* __restrict__ mst_w, const int* __restrict__ flags) {
    if (flags[CL_CNT_DONE]) return;                 // the tree was complete before this round: queued ahead without a host read
    int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    if (comp[c] != c) return;
    auto parent_of = [&](int r) { return sel_a[r] >= 0 ? comp[sel_b[r]] : r; };
    const int p = parent_of(c);
    if (p == c) { parent2[c] = c; return; }
    const bool mutual = parent_of(p) == c;
    if (mutual && c < p) {
        parent2[c] = c;            // the smaller id of a mutual pair becomes the root; its partner emits the edge
        return;
    }
    parent2[c] = p;
    int k = atomicAdd(counter, 1);
    if (k >= n - 1) return;        // only after k_cl_b_compress met a cycle (CL_CYCLE): nothing is written beyond the n - 1 edges
    mst_a[k] = perm[sel_a[c]];
    mst_b[k] = perm[sel_b[c]];
    mst_w[k] = best_w[c];
}

__global__ void k_cl_b_compress(int n, int* __restrict__ comp, const int* __restrict__ parent2, int* __restrict__ flags, int4* __restrict__ aux,
                                int* __restrict__ csize, unsigned long long* __restrict__ giant) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) flags[CL_CNT_DONE] = flags[CL_CNT_EDGES] >= n - 1;    // read by every kernel of the NEXT round (stream order): rounds are queued in
                                                // batches without a host read in between, a round after the last one is a no-op
    if (i == 0) *giant = 0ull;                   // the next round's k_cl_b_round_init takes the maximum again
    if (i >= n) return;
    const int old = comp[i];
    int r = old;
    // Picks that are each component's minimum under the strict order form no cycle except mutual pairs (k_cl_b_emit breaks those), so
    // this walk reaches a root.  A search that prunes wrongly breaks that; the walk then ends after n hops and marks the edge counter:
    // the call returns VG_ERR_HIP (every later round is a no-op: flags[CL_CNT_DONE]) instead of spinning on the device.
    int hops = 0;
    while (parent2[r] != r && hops < n) { r = parent2[r]; ++hops; }
    if (parent2[r] != r) atomicOr(&flags[CL_CNT_EDGES], CL_CYCLE);
    // an absorbed root hands its point count to the new root (only new roots are written, and a new root never reads its own count here)
    if (old == i && r != i) atomicAdd(&csize[r], csize[i]);
    comp[i] = r;
    aux[i].z = r;
}

__global__ void k_cl_iota(int n, int* p) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = i;
}

__global__ void k_cl_unsort_core(int n, const int* __restrict__ perm, const double* __restrict__ core2_s,
                                 double* __restrict__ core2_orig) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) core2_orig[perm[i]] = core2_s[i];
}

__global__ void k_cl_gather_edges(int m, const int* __restrict__ idx_s, const int* __restrict__ a,
                                  const int* __restrict__ b, int* __restrict__ lo, int* __restrict__ hi) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    int e = idx_s[i];
    int x = a[e], y = b[e];
    lo[i] = x < y ? x : y;
    hi[i] = x < y ? y : x;
}

// What an MST reads ONCE and hands to every launch of every round.  The product's values are fixed; the development build reads its
// switches into them, once per MST too -- a switch that a tool flips between a round's search and pick launches would let pick accept
// candidates of a component that did not search (ADVICE r5).
struct ClSwitches {
    int sit_min;          // smallest size at which the largest component sits a round out (k_cl_b_round_init): an eighth of the points
    int xcd_order;        // the walk's workgroups in cl_xcd_block order
    int first_batch;      // Boruvka rounds queued before the first host read of the edge counter
};

// the walk of one Boruvka round: THE launch of k_cl_b_search (the product's NT is 512: see the kernel)
template <int DIM, int NT>
static void cl_launch_walk(vg_cluster* h, int n, hipStream_t st, int sit_min, int xcd_order) {
    hipLaunchKernelGGL((k_cl_b_search<DIM, NT>), dim3(vg_div_up(n, NT)), dim3(NT), 0, st, h->d_spts, h->d_st, n, h->d_grid, h->d_cell_start,
                       h->d_cell_comp, h->d_cell_e, h->d_perm, h->d_core2, h->d_comp, h->d_aux, h->d_best_w, h->d_pt_w, h->d_pt_d, h->d_pt_key,
                       h->d_pt_b, h->d_pt_lb, h->d_dbg, h->d_counter, h->d_giant, sit_min, xcd_order);
}

#ifdef VG_DEV      // the development build's kernels, switches and simulations: cl_dev_switches, cl_dev_core_walk, cl_dev_round_search
#include "dev/cluster_dev.inc"
#endif

// vg_cluster_mst_nd behind its argument checks, for one clustering space
template <int DIM>
static int cl_mst(vg_cluster* h, const float* d_points, int n, int stride, int k, double* d_core2, int32_t* d_mst_lo, int32_t* d_mst_hi,
                  double* d_mst_w2, int32_t* h_rounds, hipStream_t st) {
    const int nb = vg_div_up(n, 256);
    {
        const int rc = cl_build_grid(h, d_points, n, stride, DIM, st);
        if (rc != VG_OK) return rc;
    }
    if (DIM >= 4) {
        hipLaunchKernelGGL(k_cl_e_leaf, dim3(nb), dim3(256), 0, st, n, h->d_code_s, h->d_spts, h->d_cell_e);
        for (int l = 1; l < CL_PUR_LEVELS; ++l)
            hipLaunchKernelGGL(k_cl_e_up, dim3(nb), dim3(256), 0, st, n, l, h->d_code_s, h->d_cell_start, h->d_cell_e);
    }
    cl_launch_core<DIM>(h, n, k, st);
    if (d_core2) hipLaunchKernelGGL(k_cl_unsort_core, dim3(nb), dim3(256), 0, st, n, h->d_perm, h->d_core2, d_core2);
    VG_LAUNCH_CHECK();
    // ---- Boruvka ----
    hipLaunchKernelGGL(k_cl_b_init, dim3(nb), dim3(256), 0, st, n, h->d_comp, h->d_counter, h->d_pt_b, h->d_pt_lb, h->d_core2,
                       DIM >= 5 ? h->d_st : (const float*)nullptr, h->d_aux, h->d_csize, h->d_giant);
    // Rounds are queued in batches WITHOUT a host read in between: every round's kernels start with `if (flags[CL_CNT_DONE]) return`,
    // and k_cl_b_compress sets flags[CL_CNT_DONE] once the n - 1 edges are out, so a round queued after the last needed one costs a
    // dozen empty launches.  The edge count of every round is copied to its own pinned slot; the host reads them once per batch
    // (first batch: CL_FIRST_BATCH rounds -- 150k-point frames need 6-8 -- then one round at a time).
    int rounds = 0, edges = 0, needed = 0;
    int* const flags = h->d_counter;
    ClSwitches sw = {std::max(2, n / 8), 1, CL_FIRST_BATCH};      // one reading per MST
#ifdef VG_DEV
    cl_dev_switches(&sw);
#endif
    auto one_round = [&](int r) {
        hipLaunchKernelGGL(k_cl_b_round_init, dim3(nb), dim3(256), 0, st, n, h->d_comp, h->d_best_w, h->d_best_d, h->d_best_e, h->d_sel_a, flags, h->d_csize, h->d_giant, h->d_code_s, h->d_cell_comp);
        if (r > 1) hipLaunchKernelGGL(k_cl_b_seed, dim3(nb), dim3(256), 0, st, n, h->d_comp, h->d_pt_b, h->d_pt_w, h->d_best_w, flags);
        hipLaunchKernelGGL(k_cl_b_purity, dim3(nb), dim3(256), 0, st, n, h->d_code_s, h->d_comp, h->d_cell_comp, flags);
#ifdef VG_DEV      // the walk at the workgroup size asked for, inside the simulations that run a round's search twice
        cl_dev_round_search<DIM>(h, n, st, r, sw);
#else
        cl_launch_walk<DIM, 512>(h, n, st, sw.sit_min, sw.xcd_order);
#endif
        hipLaunchKernelGGL(k_cl_b_select_d, dim3(nb), dim3(256), 0, st, n, h->d_comp, h->d_best_w, h->d_pt_w, h->d_pt_d, h->d_best_d, flags);
        hipLaunchKernelGGL(k_cl_b_select, dim3(nb), dim3(256), 0, st, n, h->d_comp, h->d_best_w, h->d_best_d, h->d_pt_w, h->d_pt_d,
                           h->d_pt_key, h->d_best_e, flags);
        hipLaunchKernelGGL(k_cl_b_pick, dim3(nb), dim3(256), 0, st, n, h->d_comp, h->d_best_w, h->d_best_d, h->d_best_e, h->d_pt_w,
                           h->d_pt_d, h->d_pt_key, h->d_pt_b, h->d_sel_a, h->d_sel_b, flags, h->d_giant, sw.sit_min);
        hipLaunchKernelGGL(k_cl_b_emit, dim3(nb), dim3(256), 0, st, n, h->d_comp, h->d_sel_a, h->d_sel_b, h->d_best_w,
                           h->d_perm, h->d_parent2, h->d_counter, h->d_mst_a, h->d_mst_b, h->d_mst_w, flags);
        hipLaunchKernelGGL(k_cl_b_compress, dim3(nb), dim3(256), 0, st, n, h->d_comp, h->d_parent2, flags, h->d_aux, h->d_csize, h->d_giant);
        return hipMemcpyAsync(h->h_counter + ((r - 1) & 15), h->d_counter, 4, hipMemcpyDeviceToHost, st);
    };
    while (edges < n - 1) {
        const int batch = (rounds == 0 && !h->d_dbg) ? sw.first_batch : 1;
        const int first = rounds + 1;
        for (int b = 0; b < batch; ++b) {
            if (++rounds > 64) {
                fprintf(stderr, "[vilgod_hip] vg_cluster_mst: Boruvka did not converge (%d of %d edges)\n", edges, n - 1);
                return VG_ERR_HIP;
            }
            VG_CHECK(one_round(rounds));
        }
        VG_CHECK(hipStreamSynchronize(st));
        for (int r = first; r <= rounds; ++r) {
            const int e = h->h_counter[(r - 1) & 15];
            if (h->d_dbg) {
                const ClDbgCounts sc = cl_dbg_counts(h, n, st);
                fprintf(stderr, "[cluster dbg] round %d: edges %d -> %d, searching threads %d, scanned points: total %lld, median %d, p99 %d, p99.9 %d, max %d\n",
                        r, edges, e, sc.nonzero, sc.total, sc.at(1, 2), sc.at(99, 100), sc.at(999, 1000), sc.max());
            }
            if (e == edges && !needed) {
                fprintf(stderr, "[vilgod_hip] vg_cluster_mst: no progress in round %d (%d of %d edges)\n", r, e, n - 1);
                return VG_ERR_HIP;
            }
            edges = e;
            if (edges >= n - 1 && !needed) needed = r;
        }
    }
    if (edges & CL_CYCLE) {
        fprintf(stderr, "[vilgod_hip] vg_cluster_mst: the picks of a Boruvka round formed a cycle (a pruning bound is wrong)\n");
        return VG_ERR_HIP;
    }
    rounds = needed;
    if (h_rounds) *h_rounds = rounds;
    // ---- sort edges by weight ----
    const int m = n - 1;
    hipLaunchKernelGGL(k_cl_iota, dim3(vg_div_up(m, 256)), dim3(256), 0, st, m, h->d_mst_idx);
    size_t tb = h->temp_bytes;
    VG_CHECK(rocprim::radix_sort_pairs(h->d_temp, tb, h->d_mst_w, h->d_mst_w_s, h->d_mst_idx, h->d_mst_idx_s, (size_t)m, 0, 64, st));
    if (d_mst_lo && d_mst_hi)
        hipLaunchKernelGGL(k_cl_gather_edges, dim3(vg_div_up(m, 256)), dim3(256), 0, st, m, h->d_mst_idx_s, h->d_mst_a, h->d_mst_b,
                           d_mst_lo, d_mst_hi);
    if (d_mst_w2) VG_CHECK(hipMemcpyAsync(d_mst_w2, h->d_mst_w_s, 8 * (size_t)m, hipMemcpyDeviceToDevice, st));
    VG_LAUNCH_CHECK();
    return VG_OK;
}
