// Development build only (-DVG_DEV, libvilgod_hip_dev.so): included by ../cluster.hip in place, behind cl_launch_walk.
// The per-point k-NN walk that the cooperative phases replaced (an independent reference for the A/B tools), and the switches and
// simulations of the Boruvka rounds.  cluster.hip calls in at three points: cl_dev_switches (once per MST), cl_dev_core_walk (in front of
// the core-distance phases), cl_dev_round_search (a round's search).
//   VG_CLUSTER_CORE_WALK=1     core distances by k_cl_core (k <= 15)
//   VG_CLUSTER_SITOUT=0        the largest component searches like every other
//   VG_CLUSTER_FIRST_BATCH=b   rounds queued before the first host read (1 .. 12)
//   VG_CLUSTER_XCD_ORDER=0     the walk's workgroups in hardware order
//   VG_CLUSTER_SEARCH_NT=t     threads per workgroup of the walk: 256, 512 (the product's) or 768
//   VG_CLUSTER_BOUNDSIM=1      every round's search runs twice, the second time against every component's final bound
//   VG_CLUSTER_SEEDSIM=1       round 1's search runs again for the points a k-NN seed could not serve

// the per-point tree walk of rounds 1-2 (superseded by the cooperative kernels in round 3): pruned depth-first walk of the implicit octree,
// nearest child first, box-distance pruning against the current k-th distance, nodes with <= CL_LEAF points scanned directly, a
// 16-entry register-resident sorted list (entry 0 is the point itself, so k <= 15)
template <int DIM>
__global__ __launch_bounds__(256) void k_cl_core(const float4* __restrict__ spts, const float* __restrict__ stt, int n,
                                                 const ClGrid* __restrict__ gp, const int* __restrict__ cs,
                                                 const unsigned int* __restrict__ cell_e, int k,
                                                 double* __restrict__ core2, int* __restrict__ dbg_scan) {
    __shared__ unsigned int stack[CL_STACK * 256];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int scanned = 0;                                  // VG_CLUSTER_DEBUG: pair distances evaluated by this point
    unsigned int* st = stack + threadIdx.x;
    const ClGrid g = *gp;
    const float4 qf = spts[i];
    const double qx = qf.x, qy = qf.y, qz = qf.z, qe = qf.w, qt = DIM >= 5 ? (double)stt[i] : 0.0;
    int cx, cy, cz;
    cl_cell_of(g, qx, qy, qz, cx, cy, cz);
    double h[CL_K];
#pragma unroll
    for (int j = 0; j < CL_K; ++j) h[j] = INFINITY;
    const int rx0 = cx >> CL_LMAX, ry0 = cy >> CL_LMAX;
    const int nrx = CL_NX >> CL_LMAX, nry = CL_NY >> CL_LMAX;
    for (int rr = 0; rr < nrx * nry; ++rr) {
        // own root first, then the others (pruned by distance)
        int rx = rr % nrx, ry = rr / nrx;
        if (rr == 0) { rx = rx0; ry = ry0; }
        else if (rx == rx0 && ry == ry0) { rx = 0; ry = 0; }
        int sp = 0;
        st[0] = cl_pack(CL_LMAX, rx, ry, 0);
        sp = 1;
        while (sp > 0) {
            int l, x, y, z;
            cl_unpack(st[(--sp) * 256], l, x, y, z);
            const double nb2 = cl_box_d2(g, qx, qy, qz, l, x, y, z);
            if (nb2 >= h[k]) continue;                                       // cannot lower the k-th distance (ALU only)
            const unsigned int c0 = cl_code(x << l, y << l, z << l);
            const int j0 = cl_start_l(cs, l, c0 >> (3 * l)), j1 = cl_start_l(cs, l, (c0 >> (3 * l)) + 1u);
            if (j0 == j1) continue;
            if (DIM >= 4 && l < CL_PUR_LEVELS && nb2 + cl_e_gap2(cell_e[cl_pur_off_fwd(l) + (c0 >> (3 * l))], qe) >= h[k]) continue;
            if (l == 0 || j1 - j0 <= CL_LEAF) {
                scanned += j1 - j0;
                for (int jb = j0; jb < j1; jb += 4) {                       // four independent loads per trip
                    float4 pj[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) pj[u] = spts[jb + u < j1 ? jb + u : j1 - 1];
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        const int j = jb + v;
                        if (j >= j1) continue;
                        double d2 = cl_d2<DIM>(qx, qy, qz, qe, qt, pj[v], stt, j);
                        if (d2 < h[CL_K - 1]) {
#pragma unroll
                            for (int u = 0; u < CL_K; ++u)
                                if (d2 < h[u]) { double tmp = h[u]; h[u] = d2; d2 = tmp; }
                        }
                    }
                }
                continue;
            }
            // children, nearest octant LAST on the stack -> popped first
            const int l1 = l - 1;
            const int ox = ((cx >> l1) > 2 * x) ? 1 : 0, oy = ((cy >> l1) > 2 * y) ? 1 : 0, oz = ((cz >> l1) > 2 * z) ? 1 : 0;
            const int near = ox | (oy << 1) | (oz << 2);
            // the 8 children are consecutive Morton ranges: their 9 boundaries are loaded together (independent loads), so
            // empty octants -- most of them in LiDAR data -- are never pushed and never cost a pop with two dependent loads
            int bnd[9];
#pragma unroll
            for (int c = 0; c < 9; ++c) bnd[c] = cl_start_l(cs, l1, (c0 >> (3 * l1)) + (unsigned int)c);
            unsigned int occupied = 0;                    // bit c: child c holds points (static indices only: no scratch)
#pragma unroll
            for (int c = 0; c < 8; ++c) occupied |= (bnd[c] != bnd[c + 1]) ? (1u << c) : 0u;
            for (int c = 7; c >= 0; --c) {
                const int ch = c ^ near;
                if (!((occupied >> ch) & 1u)) continue;
                const int nx = 2 * x + (ch & 1), ny = 2 * y + ((ch >> 1) & 1), nz = 2 * z + ((ch >> 2) & 1);
                if (cl_box_d2(g, qx, qy, qz, l1, nx, ny, nz) >= h[k]) continue;
                if (sp < CL_STACK) st[(sp++) * 256] = cl_pack(l1, nx, ny, nz);
            }
        }
    }
    core2[i] = h[k];
    if (dbg_scan) dbg_scan[i] = scanned;
}

// Experiment (round 5, VG_CLUSTER_SEEDSIM=1): what would round 1 of the Boruvka search cost if every point whose best edge weighs exactly its
// own core distance -- the points a pass over the k-NN shell could seed without a walk -- were answered beforehand?  After round 1's search
// the candidates of all OTHER points are dropped and the search is launched again: that second launch walks only the points a seed could
// not serve (same results; its duration in the kernel trace is the residual walk).
__global__ void k_cl_seedsim_drop(int n, const double* __restrict__ core2, const unsigned long long* __restrict__ pt_w, int* __restrict__ pt_b,
                                  int* __restrict__ counter) {
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= n) return;
    const bool seedable = pt_b[a] >= 0 && pt_w[a] == (unsigned long long)__double_as_longlong(core2[a]);
    if (!seedable) { pt_b[a] = -1; atomicAdd(&counter[CL_CNT_DEV], 1); }
}

// sit_min, xcd_order and first_batch are read HERE, once per MST, and handed to every launch of every round (ADVICE r5: a switch that a
// tool flips between a round's search and pick launches would let pick accept candidates of a component that did not search).  Read per
// call, not once per process: the A/B tools switch them inside one process.
static void cl_dev_switches(ClSwitches* sw) {
    const char* e = getenv("VG_CLUSTER_SITOUT");
    if (e && atoi(e) == 0) sw->sit_min = 0x7FFFFFFF;
    if (getenv("VG_CLUSTER_XCD_ORDER")) sw->xcd_order = atoi(getenv("VG_CLUSTER_XCD_ORDER"));
    if (getenv("VG_CLUSTER_FIRST_BATCH")) sw->first_batch = std::max(1, std::min(12, atoi(getenv("VG_CLUSTER_FIRST_BATCH"))));
}

// VG_CLUSTER_CORE_WALK=1: the core distances by the per-point walk; false when the cooperative phases are to run (switch off, or k >= 16)
template <int DIM>
static bool cl_dev_core_walk(vg_cluster* h, int n, int k, hipStream_t st) {
    static const int walk = getenv("VG_CLUSTER_CORE_WALK") ? atoi(getenv("VG_CLUSTER_CORE_WALK")) : 0;
    if (!walk || k >= CL_K) return false;
    hipLaunchKernelGGL((k_cl_core<DIM>), dim3(vg_div_up(n, 256)), dim3(256), 0, st, h->d_spts, h->d_st, n, h->d_grid, h->d_cell_start,
                       h->d_cell_e, k, h->d_core2, h->d_dbg);
    return true;
}

// VG_CLUSTER_SEARCH_NT: the walk in workgroups of 256, 512 or 768 threads (see k_cl_b_search; 768 = three waves per SIMD: <= 168 registers,
// 132 KB of stack, 103 instead of 155 workgroups for 79k points -- A/B, round 6).  Read per launch: it changes no result.
template <int DIM>
static void cl_dev_launch_walk(vg_cluster* h, int n, hipStream_t st, const ClSwitches& sw) {
    const char* nt_env = getenv("VG_CLUSTER_SEARCH_NT");
    const int nt = nt_env ? atoi(nt_env) : 512;
    if (nt == 768) cl_launch_walk<DIM, 768>(h, n, st, sw.sit_min, sw.xcd_order);
    else if (nt == 512) cl_launch_walk<DIM, 512>(h, n, st, sw.sit_min, sw.xcd_order);
    else cl_launch_walk<DIM, 256>(h, n, st, sw.sit_min, sw.xcd_order);
}

// The search of round r, between k_cl_b_purity and k_cl_b_select_d.
template <int DIM>
static void cl_dev_round_search(vg_cluster* h, int n, hipStream_t st, int r, const ClSwitches& sw) {
    const int nb = vg_div_up(n, 256);
    int* const flags = h->d_counter;
    // VG_CLUSTER_BOUNDSIM (round 6, VERDICT r5 task 6: would a component-level search pay?).  What a workgroup-per-component search adds
    // to this walk is a component bound every point sees AT ONCE (here: published through best_w by atomicMin, read at the start and every
    // 8th node).  Simulated before being built: every round's search is launched a SECOND time with best_w already holding each
    // component's final minimum (candidates and lower bounds restored to their state in front of the first launch) -- no shared bound
    // can prune more than the true one from the first node on.  The second launches' durations are the floor of that family.
    static const bool boundsim = getenv("VG_CLUSTER_BOUNDSIM") != nullptr;
    static int* sim_b = nullptr; static double* sim_lb = nullptr; static int sim_n = 0;
    if (boundsim) {
        if (sim_n < n) { (void)hipFree(sim_b); (void)hipFree(sim_lb); (void)hipMalloc(&sim_b, (size_t)n * 4); (void)hipMalloc(&sim_lb, (size_t)n * 8); sim_n = n; }
        (void)hipMemcpyAsync(sim_b, h->d_pt_b, (size_t)n * 4, hipMemcpyDeviceToDevice, st);
        (void)hipMemcpyAsync(sim_lb, h->d_pt_lb, (size_t)n * 8, hipMemcpyDeviceToDevice, st);
        cl_dev_launch_walk<DIM>(h, n, st, sw);
        // best_w now holds every component's minimum: search again from the same candidates / lower bounds (this launch's outputs are the
        // ones the round goes on with: the same edges -- tests still pass with the switch on)
        (void)hipMemcpyAsync(h->d_pt_b, sim_b, (size_t)n * 4, hipMemcpyDeviceToDevice, st);
        (void)hipMemcpyAsync(h->d_pt_lb, sim_lb, (size_t)n * 8, hipMemcpyDeviceToDevice, st);
    }
    cl_dev_launch_walk<DIM>(h, n, st, sw);
    if (r == 1 && getenv("VG_CLUSTER_SEEDSIM")) {
        (void)hipMemsetAsync(h->d_counter + CL_CNT_DEV, 0, 4, st);
        hipLaunchKernelGGL(k_cl_seedsim_drop, dim3(nb), dim3(256), 0, st, n, h->d_core2, h->d_pt_w, h->d_pt_b, h->d_counter);
        hipLaunchKernelGGL(k_cl_b_round_init, dim3(nb), dim3(256), 0, st, n, h->d_comp, h->d_best_w, h->d_best_d, h->d_best_e, h->d_sel_a, flags, h->d_csize, h->d_giant, h->d_code_s, h->d_cell_comp);
        hipLaunchKernelGGL(k_cl_b_seed, dim3(nb), dim3(256), 0, st, n, h->d_comp, h->d_pt_b, h->d_pt_w, h->d_best_w, flags);
        hipLaunchKernelGGL(k_cl_b_purity, dim3(nb), dim3(256), 0, st, n, h->d_code_s, h->d_comp, h->d_cell_comp, flags);   // (round_init rewrote the pure values)
        cl_dev_launch_walk<DIM>(h, n, st, sw);          // walks only the points that were not seedable
        int left = 0;
        (void)hipMemcpyAsync(&left, h->d_counter + CL_CNT_DEV, 4, hipMemcpyDeviceToHost, st);
        (void)hipStreamSynchronize(st);
        fprintf(stderr, "[cluster seedsim] round 1: %d of %d points have no edge at their own core distance (the second k_cl_b_search launch walks only these)\n", left, n);
    }
}
